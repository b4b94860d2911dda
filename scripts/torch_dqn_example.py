#!/usr/bin/env python3
"""A PyTorch agent on the GPU data engine (qlx_torch): a small torch.nn DQN acts on device observations,
steps the batched Breakout envs, pushes into the HBM replay, samples n-step batches and takes Adam steps, all without a
host copy of a frame.  It shows the calls in the order an agent makes them and prints loss and env-steps/s; a few hundred
updates teach nothing, and nothing here is a learning claim.

  python scripts/torch_dqn_example.py [--envs 256] [--updates 300] [--batch 64] [--n-step 3]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import qlx_torch as QT  # noqa: E402  (before any other use of qlx)


def make_net():
    return nn.Sequential(nn.Conv2d(4, 16, 8, stride=4), nn.ReLU(), nn.Conv2d(16, 32, 4, stride=2), nn.ReLU(), nn.Flatten(),
                         nn.Linear(32 * 9 * 9, 256), nn.ReLU(), nn.Linear(256, QT.TorchEnv.ACTION_SPACE))


def q_values(net, states_u8):
    return net(states_u8.float().mul_(1.0 / 255.0))


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
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    env = QT.TorchEnv(args.envs, seed=1, device=dev)
    rb = QT.TorchReplay(args.replay, env)
    online, target = make_net().to(dev), make_net().to(dev)
    target.load_state_dict(online.state_dict())
    opt = torch.optim.Adam(online.parameters(), lr=2.5e-4)

    steps = updates = 0
    last_loss = torch.zeros((), device=dev)
    t0 = time.perf_counter()
    while updates < args.updates:
        eps = max(0.1, 1.0 - updates / max(1, args.updates))
        with torch.no_grad():
            greedy = q_values(online, env.obs("nchw_time")).argmax(dim=1)
        explore = torch.rand(args.envs, device=dev) < eps
        actions = torch.where(explore, torch.randint(0, 3, (args.envs,), device=dev), greedy).to(torch.uint8)
        rewards, dones = env.step(actions)
        rb.add(env, actions, rewards, dones)
        env.reset(dones)   # finished games start again; their next transition has episode step 1
        steps += 1
        if steps < args.warmup_steps:
            continue
        b = rb.sample(args.batch, seed=42, update_idx=updates, n_step=args.n_step, gamma=args.gamma)
        with torch.no_grad():
            bootstrap = q_values(target, b.s_next).max(dim=1).values
            y = b.returns + b.discounts * bootstrap * (1.0 - b.terminals.float())
        q = q_values(online, b.s).gather(1, b.actions.long().unsqueeze(1)).squeeze(1)
        loss = nn.functional.smooth_l1_loss(q, y)
        last_loss = loss.detach()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        updates += 1
        if updates % args.target_sync == 0:
            target.load_state_dict(online.state_dict())
        if updates % 50 == 0:
            print(f"update {updates:4d}  loss {float(last_loss):.5f}  eps {eps:.2f}  replay {len(rb)}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.sync()
    rb.sync()
    print(f"done: {updates} updates, {steps} vector steps x {args.envs} envs in {dt:.2f} s = {steps * args.envs / dt:,.0f} env-steps/s "
          f"(acting net, replay and updates included), last loss {float(last_loss):.5f}")
    rb.close()
    env.close()


if __name__ == "__main__":
    main()
