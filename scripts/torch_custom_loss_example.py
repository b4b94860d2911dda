#!/usr/bin/env python3
"""The loop of torch_qlx_dqn_example.py with a loss the built-in training head cannot express (qlx_torch.TorchQNet's
autograd path): the double-DQN n-step Huber TD loss plus a CQL-style penalty alpha * mean(logsumexp_a Q(s, a) -
Q(s, a_taken)), which puts a gradient on all three Q-values of a sample.  The loss is three lines of torch; the forward, the
backward from dloss/dQ, clip and Adam run in the hand-written kernels on states that never leave the replay ring.  A few
hundred updates teach nothing, and nothing here is a learning claim.

Order matters in one place: forward, loss.backward() and step() come before the next env.step / rb.add, because the
backward reads the replay's frames in place (the net raises RuntimeError otherwise).

  python scripts/torch_custom_loss_example.py [--envs 256] [--updates 300] [--batch 64] [--n-step 3] [--arch f32|bf16] [--alpha 0.1]
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
    ap.add_argument("--alpha", type=float, default=0.1, help="weight of the logsumexp penalty")
    ap.add_argument("--warmup-steps", type=int, default=20)
    ap.add_argument("--target-sync", type=int, default=100)
    ap.add_argument("--arch", choices=("f32", "bf16"), default="f32")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    env = QT.TorchEnv(args.envs, seed=1, device=dev)
    rb = QT.TorchReplay(args.replay, env)
    reserve = max(args.envs, args.batch)
    online = QT.TorchQNet(args.arch, seed=2, env=env, reserve=reserve)    # env, replay and both nets on one stream
    target = QT.TorchQNet(args.arch, seed=3, env=env, reserve=reserve)
    target.copy_weights_from(online)
    lay = "nchw_time"   # one channel convention for every call on these nets

    steps = updates = 0
    last = torch.zeros(2, device=dev)
    t0 = time.perf_counter()
    while updates < args.updates:
        eps = max(0.1, 1.0 - updates / max(1, args.updates))
        greedy = online.q(env=env, layout=lay, want="actions")
        explore = torch.rand(args.envs, device=dev) < eps
        actions = torch.where(explore, torch.randint(0, 3, (args.envs,), device=dev, dtype=torch.uint8), greedy)
        rewards, dones = env.step(actions)
        rb.add(env, actions, rewards, dones)
        env.reset(dones)
        steps += 1
        if steps < args.warmup_steps:
            continue
        idx = rb.sample_indices(args.batch, seed=42, update_idx=updates)
        b = rb.batch(idx, n_step=args.n_step, gamma=args.gamma, layout=lay,
                     fields=("actions", "returns", "discounts", "terminals", "last_indices"))   # no state is copied
        a_star = online.q(replay=rb, indices=b.last_indices, which="s_next", layout=lay, want="actions")
        q_next = target.q(replay=rb, indices=b.last_indices, which="s_next", layout=lay, want="q")
        bootstrap = q_next.gather(1, a_star.long().unsqueeze(1)).squeeze(1)
        y = b.returns + b.discounts * bootstrap * (1.0 - b.terminals.float())
        # the differentiable forward comes last: its activations are the ones the backward reuses
        q = online(replay=rb, indices=idx, layout=lay)            # [batch, 3] with a grad_fn
        q_a = q.gather(1, b.actions.long().unsqueeze(1)).squeeze(1)
        td = torch.nn.functional.huber_loss(q_a, y, delta=1.0)
        penalty = (torch.logsumexp(q, dim=1) - q_a).mean()
        (td + args.alpha * penalty).backward()                     # dloss/dQ -> the net's backward kernels
        online.step()                                              # clip_by_norm + Adam
        last = torch.stack((td.detach(), penalty.detach()))
        updates += 1
        if updates % args.target_sync == 0:
            target.copy_weights_from(online)
        if updates % 50 == 0:
            print(f"update {updates:4d}  td {float(last[0]):.5f}  penalty {float(last[1]):.5f}  eps {eps:.2f}  replay {len(rb)}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.sync()
    rb.sync()
    online.sync()
    target.sync()
    assert online.model.iterations() == updates
    print(f"done: {updates} updates, {steps} vector steps x {args.envs} envs in {dt:.2f} s = {steps * args.envs / dt:,.0f} env-steps/s "
          f"(acting net, replay and updates included), last td {float(last[0]):.5f} penalty {float(last[1]):.5f}")
    env.close()   # closes the replay and the nets that share its stream first


if __name__ == "__main__":
    main()
