#!/usr/bin/env python3
"""A/B measurement of the per-update training metrics (DESIGN.md "Training metrics").

Shape: config C3 - 8,192 envs, a replay of 1,000,000 transitions prefilled to capacity (which also passes the 50k-step
pure-random phase), B = 1024, replay ratio 8 (64 updates per vector step) - once with the fp32 Q-net and once with bf16.
The two arms are metrics on (a ring of 4,096 rows, drained every 64 vector steps: exactly one ring) and metrics off.
One process and one learner per precision: the arms alternate on it (on, off, on, off, ..), each arm `--steps` vector
steps timed with a host clock around work that ends in a synchronise (the on arm's drains are inside its clock), after a
warm-up pair that is not counted.  Then, in a pass of its own, events around every launch of the "metrics" scope give
the kernel's own time per launch.  One JSON line per arm with every rate, and a summary line per precision with
median [min..max] env-steps/s of both arms, the ratio of the medians and whether the two ranges are separate; nothing
is asserted.

  python scripts/metrics_bench.py [--pairs 5] [--steps 64] [--envs 8192] [--replay 1000000] [--batch 1024] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))
import qlx  # noqa: E402

CAPACITY, DRAIN_EVERY = 4096, 64


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def timed_arm(L, on, steps, n_envs):
    """env-steps/s of `steps` vector steps with metrics on (drained every DRAIN_EVERY steps) or off; rows seen, dropped"""
    L.metrics_enable(CAPACITY if on else 0)
    L.sync()
    rows = dropped = 0
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(DRAIN_EVERY, steps - done)
        L.run(k)
        done += k
        if on:
            r, d = L.metrics()
            rows += len(r)
            dropped += d
    L.sync()
    dt = time.perf_counter() - t0
    return n_envs * steps / dt, rows, dropped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5, help="counted (on, off) pairs per precision, at least 5")
    ap.add_argument("--steps", type=int, default=64, help="vector steps per arm")
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--replay", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--replay-ratio", type=int, default=8)
    ap.add_argument("--scope-steps", type=int, default=8, help="vector steps of the event-timed pass")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.pairs >= 5
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    N = args.envs
    for precision, prec in (("fp32", qlx.PREC_F32), ("bf16", qlx.PREC_BF16)):
        p = qlx.Parameter(n_envs=N, batch_size=args.batch, update_after_actions=args.batch // args.replay_ratio,
                          history_buffer_len=args.replay, qnet_precision=prec, stats_after_steps=0)
        L = qlx.SelfDrivingQLearner(p)
        prefill = max(-(-args.replay // N), -(-p.epsilon_pure_random_steps // N))
        L.prefill(prefill)
        L.sync()
        for on in (True, False):   # the warm-up pair: code objects, the ring and its pinned buffer
            timed_arm(L, on, args.steps, N)
        rates = {True: [], False: []}
        rows = dropped = 0
        for _ in range(args.pairs):
            for on in (True, False):
                r, n, d = timed_arm(L, on, args.steps, N)
                rates[on].append(r)
                rows += n
                dropped += d
        # the kernel's own time: events around every launch of the scope, in a pass of its own
        L.metrics_enable(CAPACITY)
        L.profile(True)
        L.profile_filter("metrics", stride=1)
        L.run(args.scope_steps)
        L.sync()
        us, _, launches = L.profile_get("metrics")
        L.profile(False)
        st = L.stats()
        L.close()
        for on in (True, False):
            emit(dict(kind="arm", precision=precision, metrics="on" if on else "off", env_steps_per_s=rates[on],
                      **spread(rates[on])))
        a, b = spread(rates[True]), spread(rates[False])
        emit(dict(kind="summary", precision=precision, pairs=args.pairs, steps_per_arm=args.steps, envs=N, batch=args.batch,
                  replay=args.replay, prefill_vector_steps=prefill, replay_len=st["replay_len"], capacity=CAPACITY,
                  drain_every=DRAIN_EVERY, rows_read=rows, rows_dropped=dropped, on=a, off=b,
                  on_over_off=a["median"] / b["median"], ranges_separate=a["max"] < b["min"] or b["max"] < a["min"],
                  metrics_scope_us_per_launch=us / max(launches, 1), metrics_scope_launches=launches))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
