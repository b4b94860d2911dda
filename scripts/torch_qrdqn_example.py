#!/usr/bin/env python3
"""The loop of torch_qlx_dqn_example.py with a wide output head on the hand-written trunk (qlx_torch.TorchQNet.attach_head,
DESIGN.md §19) and the agent's loss written in torch: QR-DQN (Dabney et al. 2018) with a 3 x N quantile head and the
quantile-Huber loss, or, with --dueling, a 1 + 3 head with Q = V + A - mean A (Wang et al. 2016) and a Huber TD loss.

Per update: the target net's head values s' through replay indices (no_grad), the target is a few lines of torch, the
online net's forward(head=True) returns (q, z) from one trunk forward, loss.backward() runs the head's and the trunk's
backward kernels, step() clips and applies Adam to the ten variables and to the head's two.  States never leave the replay
ring.  It shows the calls in the order an agent makes them and prints loss and env-steps/s; a few hundred updates teach
nothing, and nothing here is a learning claim.

  python scripts/torch_qrdqn_example.py [--envs 256] [--updates 300] [--batch 64] [--quantiles 51] [--n-step 3] [--dueling]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

import torch  # noqa: E402
import qlx_torch as QT  # noqa: E402  (before any other use of qlx)


def quantile_huber(theta, target):
    """theta [B, N] the taken action's quantiles, target [B, N] (no grad): sum over i of the mean over j of
    |tau_i - 1{u < 0}| Huber_1(u), u = target_j - theta_i; mean over the batch"""
    n = theta.shape[1]
    u = target[:, None, :] - theta[:, :, None]
    huber = torch.where(u.abs() <= 1, 0.5 * u * u, u.abs() - 0.5)
    tau = (torch.arange(n, device=theta.device, dtype=theta.dtype) + 0.5) / n
    return ((tau[None, :, None] - (u.detach() < 0).float()).abs() * huber).mean(dim=2).sum(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--replay", type=int, default=20_000)
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--quantiles", type=int, default=51)
    ap.add_argument("--n-step", type=int, default=3)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--warmup-steps", type=int, default=20)
    ap.add_argument("--target-sync", type=int, default=100)
    ap.add_argument("--dueling", action="store_true", help="a 1 + 3 head, Q = V + A - mean A, Huber TD loss")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    N = args.quantiles
    width = 4 if args.dueling else 3 * N
    env = QT.TorchEnv(args.envs, seed=1, device=dev)
    rb = QT.TorchReplay(args.replay, env)
    reserve = max(args.envs, args.batch)
    online = QT.TorchQNet("f32", seed=2, env=env, reserve=reserve)    # env, replay and both nets on one stream
    target = QT.TorchQNet("f32", seed=3, env=env, reserve=reserve)
    online.attach_head(width, seed=4)
    target.attach_head(width, seed=5)
    target.copy_weights_from(online)   # the ten variables and the head
    lay = "nchw_time"

    def values(z):
        """Q [n, 3] of a head output: the quantile means, or V + A - mean A"""
        if args.dueling:
            adv = z[:, 1:4]
            return z[:, :1] + adv - adv.mean(dim=1, keepdim=True)
        return z.view(-1, 3, N).mean(dim=2)

    steps = updates = 0
    last_loss = torch.zeros((), device=dev)
    t0 = time.perf_counter()
    while updates < args.updates:
        eps = max(0.1, 1.0 - updates / max(1, args.updates))
        with torch.no_grad():
            _, z_env = online.forward(env=env, layout=lay, head=True)   # acting on the env's ring: nothing is copied
            greedy = values(z_env).argmax(dim=1).to(torch.uint8)
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
                     fields=("actions", "returns", "discounts", "terminals", "last_indices"))
        live = b.discounts * (1.0 - b.terminals.float())
        with torch.no_grad():
            _, z_next = target.forward(replay=rb, indices=b.last_indices, which="s_next", layout=lay, head=True)
            q_next = values(z_next)
            if args.dueling:   # double DQN: the online net picks a*, the target net values it
                _, z_on = online.forward(replay=rb, indices=b.last_indices, which="s_next", layout=lay, head=True)
                a_star = values(z_on).argmax(dim=1, keepdim=True)
                y = b.returns + live * q_next.gather(1, a_star).squeeze(1)
            else:
                a_star = q_next.argmax(dim=1)
                theta_next = z_next.view(-1, 3, N)[torch.arange(args.batch, device=dev), a_star]
                y = b.returns[:, None] + live[:, None] * theta_next   # [B, N] target quantiles
        _, z = online.forward(replay=rb, indices=idx, layout=lay, head=True)   # (q, z): one trunk forward, a grad_fn on both
        taken = b.actions.long()
        if args.dueling:
            last_loss = torch.nn.functional.huber_loss(values(z).gather(1, taken.unsqueeze(1)).squeeze(1), y, delta=1.0)
        else:
            last_loss = quantile_huber(z.view(-1, 3, N)[torch.arange(args.batch, device=dev), taken], y)
        last_loss.backward()   # the head's and the trunk's backward kernels; no dq: the 512 -> 3 head is not in this loss
        online.step()          # clip_by_norm + Adam of the ten variables and of Wh, bh
        updates += 1
        if updates % args.target_sync == 0:
            target.copy_weights_from(online)
        if updates % 50 == 0:
            print(f"update {updates:4d}  loss {float(last_loss):.5f}  eps {eps:.2f}  replay {len(rb)}", flush=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for o in (env, rb, online, target):
        o.sync()
    kind = "dueling 1 + 3 head" if args.dueling else f"QR-DQN, 3 x {N} quantile head"
    print(f"done ({kind}): {updates} updates, {steps} vector steps x {args.envs} envs in {dt:.2f} s = "
          f"{steps * args.envs / dt:,.0f} env-steps/s (acting net, replay and updates included), last loss {float(last_loss):.5f}")
    env.close()   # closes the replay and the nets that share its stream first


if __name__ == "__main__":
    main()
