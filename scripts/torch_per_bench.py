#!/usr/bin/env python3
"""Kernel times of one prioritized update at a time: the learner's sum-tree kernels driven one batch per
call (qlx.SumTree: k_per_sample at U = 1, k_per_claim, k_per_write, the full k_tree_build rebuild) beside the replay's
device calls (k_per_draw, the guarded claim / write, the same rebuild), on the same leaves: both arms start from priority 1
everywhere and make the same draws and the same priority writes, so their trees are equal throughout (each arm prints a
checksum of its final leaves).  Capacity 1,000,000, B = 1024, 8192 envs.

A third arm, `push`, is what an enabled replay adds to every push of 8192 transitions (k_per_push + the rebuild).

Each arm is profiled in a run of its own, kernel trace only (no counters):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/old -o t -- python scripts/torch_per_bench.py old
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/new -o t -- python scripts/torch_per_bench.py new
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/push -o t -- python scripts/torch_per_bench.py push
  python scripts/torch_per_bench.py table DIR/old DIR/new DIR/push      (reads the *_kernel_stats.csv; needs no GPU)
The table gives per kernel the calls, the average and the min..max of the stats file, and the per-update sum
draw + write + rebuild of the old and the new arm."""
import argparse
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

import numpy as np  # noqa: E402

SEED, BETA, ALPHA, EPS = 42, 0.4, 0.6, 1e-6


def td_of(rng, batch):
    return rng.gamma(0.4, 1.0, batch).astype(np.float32)


def old(args):
    import qlx
    t = qlx.SumTree(args.capacity)
    t.set_leaves(np.ones(args.capacity, np.float32))
    rng = np.random.default_rng(0)
    for u in range(args.reps):
        slots, _ = t.sample(SEED, u, 1, 0, args.capacity, BETA, args.batch)
        t.update(slots[0], td_of(rng, args.batch), ALPHA, EPS)
    leaves, total, pmax = t.get()
    print(f"old arm: {args.reps} x (sample, update); total {total!r} per_max {pmax!r} leaves sha1 {hashlib.sha1(leaves.tobytes()).hexdigest()}")
    t.close()


def new(args, pushes=False):
    import torch
    import qlx_torch as QT   # before any other use of qlx
    dev = torch.device("cuda:0")
    env = QT.TorchEnv(args.envs, seed=1, device=dev)
    rb = QT.TorchReplay(args.capacity, env)
    actions = (torch.arange(args.envs, device=dev) % 3).to(torch.uint8)

    def push():
        r, d = env.step(actions)
        rb.add(env, actions, r, d)

    while len(rb) < args.capacity:
        push()
    rb.enable_priorities()
    if pushes:
        for _ in range(args.reps):   # k_per_push + a rebuild after each push of `envs` transitions
            push()
        env.sync()
        rb.sync()
        print(f"push arm: {args.reps} pushes of {args.envs} transitions on an enabled replay")
        env.close()
        return
    rng = np.random.default_rng(0)
    tds = [torch.as_tensor(td_of(rng, args.batch)).to(dev) for _ in range(args.reps)]
    for u in range(args.reps):
        idx, _ = rb.sample_prioritized(args.batch, SEED, u, BETA)
        rb.update_priorities(idx, tds[u], ALPHA, EPS)
    rb.sync()
    p = rb.priorities()
    print(f"new arm: {args.reps} x (sample_prioritized, update_priorities); total {float(p['total'])!r} per_max {float(p['per_max'])!r} "
          f"leaves sha1 {hashlib.sha1(p['leaves'].tobytes()).hexdigest()}")
    env.close()


ROWS = {   # arm -> (kernel-name substring, launches per update (0: after a push, not part of the sum), part)
    "old": [("k_per_sample", 1, "draw"), ("k_per_claim", 1, "write"), ("k_per_write", 1, "write"), ("k_tree_build", 2, "rebuild")],
    "new": [("k_per_draw", 1, "draw"), ("k_per_claim_guarded", 1, "write"), ("k_per_write_guarded", 1, "write"),
            ("k_tree_build", 2, "rebuild")],
    "push": [("k_replay_push", 1, "the push itself"), ("k_per_push", 1, "priorities"), ("k_tree_build", 2, "rebuild")],
}


def kernel_of(name):
    """'void qlx::k_per_draw<1>(float const*, ...)' -> 'k_per_draw'"""
    return name.split("(")[0].split("<")[0].split("::")[-1].split()[-1]


def stats_of(path):
    files = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{path}: expected one *kernel_stats.csv, found {len(files)}")
    with open(files[0]) as f:
        return list(csv.DictReader(f))


def table(args):
    print("| arm | kernel | part | calls | avg us | min..max us | per update |")
    print("|---|---|---|---|---|---|---|")
    for arm, path in zip(("old", "new", "push"), args.dirs):
        rows = stats_of(path)
        total = 0.0
        for sub, per_update, part in ROWS[arm]:
            hit = [r for r in rows if kernel_of(r["Name"]) == sub]
            if not hit:
                print(f"| {arm} | {sub} | {part} | 0 | - | - | - |")
                continue
            calls = sum(int(r["Calls"]) for r in hit)
            avg = sum(float(r["TotalDurationNs"]) for r in hit) / calls / 1e3
            lo, hi = min(float(r["MinNs"]) for r in hit) / 1e3, max(float(r["MaxNs"]) for r in hit) / 1e3
            total += per_update * avg
            print(f"| {arm} | {sub} | {part} | {calls} | {avg:.2f} | {lo:.2f}..{hi:.2f} | {per_update} x |")
        print(f"| {arm} | **{'per push' if arm == 'push' else 'draw + write + rebuild per update'}** | | | **{total:.2f}** | | |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("old", "new", "push", "table"))
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    if args.what == "table" and len(args.dirs) not in (2, 3):
        ap.error("table needs the output directories of the old and the new arm (and the push arm's)")
    {"old": old, "new": new, "push": lambda a: new(a, pushes=True), "table": table}[args.what](args)


if __name__ == "__main__":
    main()
