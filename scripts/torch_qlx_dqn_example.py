#!/usr/bin/env python3
"""The loop of torch_dqn_example.py with this project's Q-net kernels in place of the torch.nn net (qlx_torch.TorchQNet,
DESIGN.md §16): the online net acts on the env's ring, the bootstrap reads s' through replay indices, a double-DQN n-step
target is computed in a few lines of torch, and forward, backward, clip and Adam of the update run in the hand-written
kernels on states that never leave the replay ring.  It shows the calls in the order an agent makes them and prints loss and
env-steps/s; a few hundred updates teach nothing, and nothing here is a learning claim.

--per draws the batch in proportion to the priorities instead: sample_prioritized, batch, targets, train
with the importance weights and want_td_abs, update_priorities - before the next add, which moves the logical indices of a
full ring - then add; none of these calls synchronises or copies to the host.

  python scripts/torch_qlx_dqn_example.py [--envs 256] [--updates 300] [--batch 64] [--n-step 3] [--arch f32|bf16] [--per]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

import torch  # noqa: E402
import qlx_torch as QT  # noqa: E402  (before any other use of qlx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--replay", type=int, default=20_000)
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-step", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--warmup-steps", type=int, default=20)
    ap.add_argument("--target-sync", type=int, default=100)
    ap.add_argument("--arch", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--per", action="store_true", help="prioritized replay: sample_prioritized / update_priorities")
    ap.add_argument("--per-alpha", type=float, default=0.6)
    ap.add_argument("--per-beta", type=float, default=0.4)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    env = QT.TorchEnv(args.envs, seed=1, device=dev)
    rb = QT.TorchReplay(args.replay, env)
    if args.per:
        rb.enable_priorities()   # every transition added from here on enters at the largest priority so far
    reserve = max(args.envs, args.batch)
    online = QT.TorchQNet(args.arch, seed=2, env=env, reserve=reserve)    # env, replay and both nets on one stream
    target = QT.TorchQNet(args.arch, seed=3, env=env, reserve=reserve)
    target.copy_weights_from(online)
    lay = "nchw_time"   # one channel convention for every call on these nets

    steps = updates = 0
    last_loss = torch.zeros((), device=dev)
    t0 = time.perf_counter()
    while updates < args.updates:
        eps = max(0.1, 1.0 - updates / max(1, args.updates))
        greedy = online.q(env=env, layout=lay, want="actions")
        explore = torch.rand(args.envs, device=dev) < eps
        actions = torch.where(explore, torch.randint(0, 3, (args.envs,), device=dev, dtype=torch.uint8), greedy)
        rewards, dones = env.step(actions)
        rb.add(env, actions, rewards, dones)
        env.reset(dones)   # finished games start again; their next transition has episode step 1
        steps += 1
        if steps < args.warmup_steps:
            continue
        if args.per:
            idx, weights = rb.sample_prioritized(args.batch, seed=42, update_idx=updates, beta=args.per_beta)
        else:
            idx, weights = rb.sample_indices(args.batch, seed=42, update_idx=updates), None
        b = rb.batch(idx, n_step=args.n_step, gamma=args.gamma, layout=lay,
                     fields=("actions", "returns", "discounts", "terminals", "last_indices"))   # no state is copied
        # double DQN over the n-step window: the online net picks a*, the target net values it
        a_star = online.q(replay=rb, indices=b.last_indices, which="s_next", layout=lay, want="actions")
        q_next = target.q(replay=rb, indices=b.last_indices, which="s_next", layout=lay, want="q")
        bootstrap = q_next.gather(1, a_star.long().unsqueeze(1)).squeeze(1)
        y = b.returns + b.discounts * bootstrap * (1.0 - b.terminals.float())
        last_loss, td_abs = online.train(b.actions, y, weights, replay=rb, indices=idx, layout=lay, want_td_abs=args.per)
        if args.per:
            rb.update_priorities(idx, td_abs, alpha=args.per_alpha)   # before the next add
        updates += 1
        if updates % args.target_sync == 0:
            target.copy_weights_from(online)
        if updates % 50 == 0:
            print(f"update {updates:4d}  loss {float(last_loss):.5f}  eps {eps:.2f}  replay {len(rb)}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.sync()
    rb.sync()
    online.sync()
    target.sync()
    print(f"done ({'prioritized' if args.per else 'uniform'} replay): {updates} updates, {steps} vector steps x {args.envs} envs in {dt:.2f} s = {steps * args.envs / dt:,.0f} env-steps/s "
          f"(acting net, replay and updates included), last loss {float(last_loss):.5f}")
    env.close()   # closes the replay and the nets that share its stream first


if __name__ == "__main__":
    main()
