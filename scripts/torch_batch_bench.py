#!/usr/bin/env python3
"""Measurement of the device-tensor batch path: qlx_replay_batch_dev against the host path it stands beside.

One process.  8,192 real envs are stepped with random device actions (finished games reset by device mask) until the
replay holds `--replay` transitions (default 204,800 = 1.4 GB of frames, past the Infinity Cache).  Then
  1. qlx_replay_batch_dev at B = `--batch` for n_step 1 and 3 in both layouts, every output asked for, into tensors
     allocated once: `--repeats` rounds, the four arms alternating inside a round, each arm `--calls` calls between two
     device events on torch's current stream; per call = the round's time / calls.  Bytes per call = frames actually read
     (non-zero channels of s and s', counted on the device) x 7,056 + 2 x B x 28,224 written.
  2. the host path for the same indices: ReplayBuffer.get_many + torch.from_numpy(..).to(device) for s and s', host
     clock around a synchronise, `--host-calls` calls.
  3. the acting loop: step + add + obs with random device actions from torch, `--act-steps` vector steps per round,
     env-steps/s of the data engine alone.
One JSON line per result; nothing is asserted.

Kernel time comes from a profiler run of its own:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python scripts/torch_batch_bench.py --profile-pass
  python scripts/torch_batch_bench.py --summarise DIR
The profile pass runs 5 + `--calls` calls per arm in the order of ARMS and 3 host get_many calls, nothing else; the
summary cuts the kernel trace by that order: k_unpack_states per arm, and the two k_replay_view launches of a get_many
summed, each as min / median / max over launches.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

ARMS = [(1, "nchw_time"), (1, "nhwc_slot"), (3, "nchw_time"), (3, "nhwc_slot")]
PROFILE_WARM, HOST_PROFILE_CALLS = 5, 3
STATE = 28224
GAMMA = 0.99


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def summarise(root, calls):
    traces = glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True)
    assert traces, f"no kernel trace under {root}"
    new, old = [], []
    for f in traces:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            row = (int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, name)
            if "k_unpack_states" in name and "ReplaySource" in name:
                new.append(row)
            elif "k_replay_view" in name:
                old.append(row)
    new.sort()
    old.sort()
    per = PROFILE_WARM + calls
    assert len(new) == per * len(ARMS), (len(new), per)
    for i, (n_step, layout) in enumerate(ARMS):
        us = [u for _, u, _ in new[i * per + PROFILE_WARM:(i + 1) * per]]
        print(json.dumps(dict(kind="kernel_new", n_step=n_step, layout=layout, launches=len(us), us=spread(us))))
    pairs = [old[i][1] + old[i + 1][1] for i in range(0, len(old) - 1, 2)]
    print(json.dumps(dict(kind="kernel_old_two_k_replay_view", get_many_calls=len(pairs), us=spread(pairs),
                          single_launch_us=spread([u for _, u, _ in old]))))
    worst_new = max(u for _, u, _ in new)
    print(json.dumps(dict(kind="kernel_bar", new_max_us=worst_new, old_pair_min_us=min(pairs),
                          ranges_separate=worst_new < min(pairs), old_over_new_medians=statistics.median(pairs) /
                          statistics.median([u for _, u, _ in new]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--replay", type=int, default=204_800)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=50, help="calls per arm and round")
    ap.add_argument("--repeats", type=int, default=5, help="rounds (calls x repeats >= 200 timed calls per arm)")
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--act-steps", type=int, default=50)
    ap.add_argument("--profile-pass", action="store_true")
    ap.add_argument("--summarise", default=None, metavar="DIR")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.calls)

    import numpy as np
    import torch
    import qlx_torch as QT

    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    dev = torch.device("cuda:0")
    N, B = args.envs, args.batch
    env = QT.TorchEnv(N, device=dev)
    rb = QT.TorchReplay(args.replay, env)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def act_step(want_obs):
        a = torch.randint(0, 3, (N,), device=dev, generator=gen, dtype=torch.uint8)
        r, d = env.step(a)
        rb.add(env, a, r, d)
        env.reset(d)   # finished games start again
        return env.obs("nchw_time") if want_obs else None

    fill = -(-args.replay // N)
    for _ in range(fill):
        act_step(False)
    env.sync()
    rb.sync()
    assert len(rb) == args.replay

    index_sets = [rb.sample_indices(B, 1234, u) for u in range(16)]
    outs = {}
    for n_step, layout in ARMS:
        shape = (B, 4, 84, 84) if layout == "nchw_time" else (B, 84, 84, 4)
        outs[n_step, layout] = dict(s=torch.empty(shape, dtype=torch.uint8, device=dev), s_next=torch.empty(shape, dtype=torch.uint8, device=dev),
                                    actions=torch.empty(B, dtype=torch.uint8, device=dev), returns=torch.empty(B, device=dev),
                                    discounts=torch.empty(B, device=dev), terminals=torch.empty(B, dtype=torch.uint8, device=dev),
                                    last_indices=torch.empty(B, dtype=torch.int64, device=dev), steps=torch.empty(B, dtype=torch.int32, device=dev))

    def run_arm(arm, calls, first=0):
        n_step, layout = arm
        for c in range(calls):
            rb.batch(index_sets[(first + c) % len(index_sets)], n_step, GAMMA, layout, out=outs[arm])

    if args.profile_pass:
        for arm in ARMS:
            run_arm(arm, PROFILE_WARM + args.calls)
            torch.cuda.synchronize()
        for c in range(HOST_PROFILE_CALLS):
            rb._rb.get_many(index_sets[c].cpu().numpy().astype(np.uint64))
        rb.sync()
        return

    # frames actually read per call, averaged over the index sets (a real frame always shows the panel: never all zero)
    frames = {}
    for n_step in (1, 3):
        tot = 0
        for idx in index_sets:
            b = rb.batch(idx, n_step, GAMMA, "nchw_time", fields=("s", "s_next"))
            tot += int(b.s.view(B, 4, -1).any(dim=2).sum()) + int(b.s_next.view(B, 4, -1).any(dim=2).sum())
        frames[n_step] = tot / len(index_sets)

    for arm in ARMS:
        run_arm(arm, 10)
    torch.cuda.synchronize()
    per_call = {arm: [] for arm in ARMS}
    for rep in range(args.repeats):
        for arm in ARMS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run_arm(arm, args.calls, first=rep)
            e1.record()
            e1.synchronize()
            per_call[arm].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    rb.sync()
    for arm in ARMS:
        n_step, layout = arm
        nbytes = frames[n_step] * 7056 + 2 * B * STATE
        us = spread(per_call[arm])
        emit(dict(kind="batch_dev", n_step=n_step, layout=layout, batch=B, replay_len=len(rb), rounds=args.repeats,
                  calls_per_round=args.calls, event_us_per_call=us, rounds_us=per_call[arm], frames_read_per_call=frames[n_step],
                  algorithmic_bytes=nbytes, tb_per_s_at_median=nbytes / us["median"] / 1e6,
                  fraction_of_6_29_copy=nbytes / us["median"] / 1e6 / 6.29, fraction_of_5_5_gather=nbytes / us["median"] / 1e6 / 5.5))

    # the host path for the same batch
    host_ms = []
    for c in range(args.host_calls + 1):
        idx = index_sets[c % len(index_sets)].cpu().numpy().astype(np.uint64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = rb._rb.get_many(idx)
        s = torch.from_numpy(g["state"]).to(dev)
        sn = torch.from_numpy(g["state_next"]).to(dev)
        torch.cuda.synchronize()
        if c:   # the first call is the warm-up
            host_ms.append((time.perf_counter() - t0) * 1e3)
        del s, sn
    emit(dict(kind="host_path", batch=B, calls=args.host_calls, end_to_end_ms=spread(host_ms),
              over_batch_dev_n1_nhwc=statistics.median(host_ms) * 1e3 / statistics.median(per_call[1, "nhwc_slot"])))

    # the acting loop
    for _ in range(10):
        act_step(True)
    torch.cuda.synchronize()
    rates = []
    for rep in range(args.repeats):
        t0 = time.perf_counter()
        for _ in range(args.act_steps):
            o = act_step(True)
        torch.cuda.synchronize()
        rates.append(N * args.act_steps / (time.perf_counter() - t0))
    del o
    env.sync()
    emit(dict(kind="acting_loop", envs=N, vector_steps_per_round=args.act_steps, rounds=args.repeats,
              loop="randint + step + add + reset(dones) + obs(nchw_time)", env_steps_per_s=spread(rates), rounds_rates=rates))
    rb.close()
    env.close()
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
