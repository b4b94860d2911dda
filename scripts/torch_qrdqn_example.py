#!/usr/bin/env python3
"""The loop of torch_qlx_dqn_example.py with a wide output head on the hand-written trunk (qlx_torch.TorchQNet.attach_head,
DESIGN.md §19) and the agent's loss written in torch: QR-DQN (Dabney et al. 2018) with a 3 x N quantile head and the
quantile-Huber loss, or, with --dueling, a 1 + 3 head with Q = V + A - mean A (Wang et al. 2016) and a Huber TD loss.

Per update: the target net's head values s' through replay indices (no_grad), the target is a few lines of torch, the
online net's forward(head=True) returns (q, z) from one trunk forward, loss.backward() runs the head's and the trunk's
backward kernels, step() clips and applies Adam to the ten variables and to the head's two.  States never leave the replay
ring.  It shows the calls in the order an agent makes them and prints loss and env-steps/s; a few hundred updates teach
nothing, and nothing here is a learning claim.

--fused keeps the same agent on the library's distributional calls: head_values() turns the head output
into greedy actions, train_dist() is the whole update - forward, quantile-Huber (or, with --c51, the projected
cross-entropy of a categorical head on [--v-min, --v-max]), backward, clip and Adam - in one enqueue-only call, fed by the
replay's batch tensors as they are.  --c51 without --fused writes that loss in torch.  --per draws prioritized batches and
feeds the per-sample loss back as the priority (either path).

--act-fused acts through TorchQNet.act(): the head's forward, its values, the argmax and the epsilon draw
(Philox, by env and step) in one call, in place of forward(head=True) + head_values() + torch.rand / torch.where.  --eval N
plays one episode in each of N fresh envs with the trained head's greedy policy at the end (qlx.Evaluator through
TorchQNet.evaluate) and prints the summary.

  python scripts/torch_qrdqn_example.py [--envs 256] [--updates 300] [--batch 64] [--quantiles 51] [--n-step 3] [--dueling]
                                        [--fused] [--c51 [--v-min -10] [--v-max 10]] [--per] [--act-fused] [--eval N]
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


def quantile_huber_samples(theta, target):
    """quantile_huber before the mean over the batch: [B]"""
    n = theta.shape[1]
    u = target[:, None, :] - theta[:, :, None]
    huber = torch.where(u.abs() <= 1, 0.5 * u * u, u.abs() - 0.5)
    tau = (torch.arange(n, device=theta.device, dtype=theta.dtype) + 0.5) / n
    return ((tau[None, :, None] - (u.detach() < 0).float()).abs() * huber).mean(dim=2).sum(dim=1)


def c51_samples(logits, logits_next, returns, live, atoms, v_min, v_max):
    """the categorical loss per sample [B]: logits [B, N] of the taken action, logits_next [B, N] of a* under the target
    net (no grad); the target distribution is the projection of returns + live z onto the atoms, in its gather form
    m_i = sum_k p'_k max(0, 1 - |Tz_k - z_i| / delta)"""
    delta = (v_max - v_min) / (atoms.numel() - 1)
    tz = (returns[:, None] + live[:, None] * atoms[None, :]).clamp(v_min, v_max)
    hat = (1.0 - (tz[:, None, :] - atoms[None, :, None]).abs() / delta).clamp(min=0.0)
    m = (torch.softmax(logits_next, dim=1)[:, None, :] * hat).sum(dim=2)
    return -(m * torch.log_softmax(logits, dim=1)).sum(dim=1)


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
    ap.add_argument("--fused", action="store_true", help="head_values() for acting and train_dist() for the update")
    ap.add_argument("--c51", action="store_true", help="a 3 x N categorical head on [--v-min, --v-max] (C51)")
    ap.add_argument("--v-min", type=float, default=-10.0)
    ap.add_argument("--v-max", type=float, default=10.0)
    ap.add_argument("--per", action="store_true", help="prioritized batches; the per-sample loss is the priority")
    ap.add_argument("--act-fused", action="store_true", help="act() for acting: forward, values, argmax and epsilon draw in one call")
    ap.add_argument("--eval", type=int, default=0, metavar="N", help="evaluate the head's greedy policy on N fresh envs at the end")
    ap.add_argument("--eval-max-steps", type=int, default=2000)
    args = ap.parse_args()
    if args.dueling and (args.fused or args.c51 or args.per or args.act_fused or args.eval):
        ap.error("--dueling goes with none of --fused, --c51, --per, --act-fused and --eval")

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
    dist = QT.Categorical(N, args.v_min, args.v_max) if args.c51 else QT.Quantile(N)
    atoms = torch.linspace(args.v_min, args.v_max, N, device=dev) if args.c51 else None
    if args.per:
        rb.enable_priorities()

    def values(z):
        """Q [n, 3] of a head output: the quantile means, the expectation of the atoms, or V + A - mean A"""
        if args.dueling:
            adv = z[:, 1:4]
            return z[:, :1] + adv - adv.mean(dim=1, keepdim=True)
        if args.c51:
            return (torch.softmax(z.view(-1, 3, N), dim=2) * atoms).sum(dim=2)
        return z.view(-1, 3, N).mean(dim=2)

    steps = updates = 0
    last_loss = torch.zeros((), device=dev)
    t0 = time.perf_counter()
    while updates < args.updates:
        eps = max(0.1, 1.0 - updates / max(1, args.updates))
        if args.act_fused:   # one call, no torch op: the draws are Philox streams by (seed, env, step)
            actions = online.act(dist, eps, 7, steps, env=env, layout=lay)
        else:
            with torch.no_grad():
                _, z_env = online.forward(env=env, layout=lay, head=True)   # acting on the env's ring: nothing is copied
                greedy = online.head_values(z_env, dist, want="actions") if args.fused else values(z_env).argmax(dim=1).to(torch.uint8)
            explore = torch.rand(args.envs, device=dev) < eps
            actions = torch.where(explore, torch.randint(0, 3, (args.envs,), device=dev, dtype=torch.uint8), greedy)
        rewards, dones = env.step(actions)
        rb.add(env, actions, rewards, dones)
        env.reset(dones)
        steps += 1
        if steps < args.warmup_steps:
            continue
        if args.per:
            idx, is_w = rb.sample_prioritized(args.batch, seed=42, update_idx=updates)
        else:
            idx, is_w = rb.sample_indices(args.batch, seed=42, update_idx=updates), None
        b = rb.batch(idx, n_step=args.n_step, gamma=args.gamma, layout=lay,
                     fields=("actions", "returns", "discounts", "terminals", "last_indices"))
        if args.fused:
            with torch.no_grad():
                _, z_next = target.forward(replay=rb, indices=b.last_indices, which="s_next", layout=lay, head=True)
            # a*, the target, the loss, both backwards, clip and Adam: one call, no torch op on the way
            last_loss, sample_loss = online.train_dist(dist, b.actions, b.returns, b.discounts, b.terminals, z_next,
                                                       weights=is_w, replay=rb, indices=idx, layout=lay,
                                                       want_sample_loss=args.per)
            if args.per:
                rb.update_priorities(idx, sample_loss)
            updates += 1
            if updates % args.target_sync == 0:
                target.copy_weights_from(online)
            if updates % 50 == 0:
                print(f"update {updates:4d}  loss {float(last_loss):.5f}  eps {eps:.2f}  replay {len(rb)}", flush=True)
            continue
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
        rows = torch.arange(args.batch, device=dev)
        if args.dueling:
            last_loss = torch.nn.functional.huber_loss(values(z).gather(1, taken.unsqueeze(1)).squeeze(1), y, delta=1.0)
        elif args.c51 or args.per:
            if args.c51:
                samples = c51_samples(z.view(-1, 3, N)[rows, taken], theta_next, b.returns, live, atoms, args.v_min, args.v_max)
            else:
                samples = quantile_huber_samples(z.view(-1, 3, N)[rows, taken], y)
            last_loss = (samples if is_w is None else is_w * samples).mean()
            if args.per:
                rb.update_priorities(idx, samples.detach())
        else:
            last_loss = quantile_huber(z.view(-1, 3, N)[rows, taken], y)
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
    kind = "dueling 1 + 3 head" if args.dueling else f"C51, 3 x {N} categorical head" if args.c51 else f"QR-DQN, 3 x {N} quantile head"
    kind += (", fused update" if args.fused else ", loss in torch") + (", prioritized" if args.per else "")
    print(f"done ({kind}): {updates} updates, {steps} vector steps x {args.envs} envs in {dt:.2f} s = "
          f"{steps * args.envs / dt:,.0f} env-steps/s (acting net, replay and updates included), last loss {float(last_loss):.5f}")
    if args.eval:
        import qlx
        ev = qlx.Evaluator(args.eval, episodes_per_env=1, max_steps_per_episode=args.eval_max_steps)
        s = online.evaluate(ev, dist)
        print(f"evaluation (greedy, {args.eval} envs x 1 episode, at most {args.eval_max_steps} steps): mean return "
              f"{s['mean_return']:.3f} [{s['min_return']:.0f}, {s['max_return']:.0f}], mean length {s['mean_length']:.1f}, "
              f"mean max-Q {s['mean_max_q']:.4f}, actions {s['action_counts'].tolist()}, {s['vector_steps']} vector steps, "
              f"{s['forward_samples']} forward rows")
        ev.close()
    env.close()   # closes the replay and the nets that share its stream first


if __name__ == "__main__":
    main()
