#!/usr/bin/env python3
"""Timings of the Q-net's device-tensor calls (qlx_torch.TorchQNet) beside the paths they replace.

  python scripts/torch_qnet_bench.py act    [--envs 8192] [--arch f32|bf16]   q(env=) | q(env.obs()) | host predict
  python scripts/torch_qnet_bench.py update [--batch 1024] [--arch f32|bf16]  train(replay=) | batch + train(obs=) | host train
  python scripts/torch_qnet_bench.py grad   [--batch 1024] [--arch f32|bf16]  a loss written in torch:
      net(replay=) + torch Huber + backward() + step(), reusing the forward's activations and recomputing them, |
      train(replay=); `--reps 0 --kernels N` only runs N of each for a kernel trace
  python scripts/torch_qnet_bench.py head   [--batch 1024] [--widths 4,153,600]   the wide output head:
      net(replay=, head=True) + a loss in torch + backward() + step() per width, beside `grad`'s update without a head on
      the same states; `--kernels N` only runs N of each width for a kernel trace (k_headw_fwd / _dz / _wgrad)
  python scripts/torch_qnet_bench.py dist   [--batch 1024]   distributional updates on the wide head, off
      the replay ring: quantile N = 51 and 200, categorical N = 51; per case forward(head=True) + the loss in torch +
      backward() + step() against train_dist(), alternated call by call, median [min..max] of 30 after 5 warm-ups, beside
      `grad`'s update without a head; `--kernels N` only runs N of each for a kernel trace (k_dist_loss_* / k_dist_values)
  python scripts/torch_qnet_bench.py head_act [--ns 256,8192]   acting with a distributional head, on an env's
      ring: act() against forward(head=True) + head_values() + the torch epsilon mix (rand, randint, where), quantile and
      categorical N = 51 per n, alternated call by call, median [min..max] of 30 after 5 warm-ups
  python scripts/torch_qnet_bench.py pack   [--n 1024]     the two staging kernels, to be run under a kernel trace:
      rocprofv3 --kernel-trace --stats -d DIR -- python scripts/torch_qnet_bench.py pack --n 8192
      (k_pack_states: the dense source of q(); k_pack_obs: the host call qlx_model_predict on the same states)

Device paths are timed with events on torch's current stream around one call (every call makes that stream wait for the
model's), host paths with a wall clock around the synchronising call; each figure is the median [min..max] of --reps
calls after --warmup calls."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "q-learning_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import qlx_torch as QT  # noqa: E402  (before any other use of qlx)

DEV = torch.device("cuda:0")


def fmt(us):
    return f"{statistics.median(us):9.1f} us [{min(us):.1f}..{max(us):.1f}]"


def time_device(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return out


def time_host(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e6)
    return out


def played_env(n, steps, rb=None):
    env = QT.TorchEnv(n, seed=1, device=DEV)
    rb = QT.TorchReplay(rb, env) if rb else None
    g = torch.Generator(device=DEV).manual_seed(0)
    for _ in range(steps):
        a = torch.randint(0, 3, (n,), device=DEV, dtype=torch.uint8, generator=g)
        r, d = env.step(a)
        if rb is not None:
            rb.add(env, a, r, d)
        env.reset(d)
    env.sync()
    return env, rb


def act(args):
    env, _ = played_env(args.envs, 12)
    net = QT.TorchQNet(args.arch, env=env, reserve=args.envs)
    lay = "nhwc_slot"
    rows = [("q(env=env)", time_device(lambda: net.q(env=env, layout=lay, want="actions"), args.reps, args.warmup)),
            ("q(env.obs())", time_device(lambda: net.q(env.obs(lay), layout=lay, want="actions"), args.reps, args.warmup)),
            ("host predict(env.state())", time_host(lambda: net.model.q_values(env._env.state()), max(3, args.reps // 4), 1))]
    print(f"acting, {args.envs} envs, {args.arch}:")
    for name, us in rows:
        print(f"  {name:28s} {fmt(us)}")
    net.sync()
    env.close()


def update(args):
    B = args.batch
    env, rb = played_env(256, 40, rb=20_000)
    net = QT.TorchQNet(args.arch, env=env, reserve=B)
    lay = "nhwc_slot"
    idx = rb.sample_indices(B, seed=3, update_idx=0)
    b = rb.batch(idx, layout=lay, fields=("s", "actions"))
    y = torch.randn(B, device=DEV)
    s_host, a_host, y_host = b.s.cpu().numpy(), b.actions.cpu().numpy(), y.cpu().numpy()

    def by_obs():
        s = rb.batch(idx, layout=lay, fields=("s",)).s
        net.train(b.actions, y, obs=s, layout=lay)

    rows = [("train(replay=, indices=)", time_device(lambda: net.train(b.actions, y, replay=rb, indices=idx, layout=lay), args.reps, args.warmup)),
            ("rb.batch + train(obs=)", time_device(by_obs, args.reps, args.warmup)),
            ("host qlx_model_train", time_host(lambda: net.model.train(s_host, a_host, y_host), max(3, args.reps // 4), 1))]
    print(f"update, B = {B}, {args.arch}:")
    for name, us in rows:
        print(f"  {name:28s} {fmt(us)}")
    net.sync()
    env.close()


def grad(args):
    B = args.batch
    env, rb = played_env(256, 40, rb=20_000)
    net = QT.TorchQNet(args.arch, env=env, reserve=B)
    lay = "nhwc_slot"
    idx = rb.sample_indices(B, seed=3, update_idx=0)
    a = rb.batch(idx, layout=lay, fields=("actions",)).actions
    a_idx = a.long().unsqueeze(1)
    y = torch.randn(B, device=DEV)

    def own_loss():
        q = net(replay=rb, indices=idx, layout=lay)
        loss = torch.nn.functional.huber_loss(q.gather(1, a_idx).squeeze(1), y, delta=1.0)
        loss.backward()
        net.step()

    def builtin():
        net.train(a, y, replay=rb, indices=idx, layout=lay)

    if args.kernels:   # for rocprofv3 --kernel-trace --stats: the same launches, untimed
        for _ in range(args.kernels):
            own_loss()
            builtin()
        net.sync()
        env.close()
        return
    rows = []
    for name, reuse in (("forward + Huber + backward + step", True), ("the same, activations recomputed", False)):
        net.reuse_activations = reuse
        rows.append((name, time_device(own_loss, args.reps, args.warmup)))
    rows.append(("train(replay=, indices=)", time_device(builtin, args.reps, args.warmup)))
    print(f"own loss, B = {B}, {args.arch}:")
    for name, us in rows:
        print(f"  {name:34s} {fmt(us)}")
    net.sync()
    env.close()


def head_loss(width, q, z, a_idx, y, dist):
    """the loss a head of this width is for, cheap enough that the kernels stay visible: 1 + 3 outputs are a dueling head
    (Q = V + A - mean A, Huber TD), 3 N outputs a categorical one (cross-entropy of the taken action's N logits against a
    fixed target distribution, the shape of C51's projected target)"""
    if width == 4:
        adv = z[:, 1:4]
        qd = z[:, :1] + adv - adv.mean(dim=1, keepdim=True)
        return torch.nn.functional.huber_loss(qd.gather(1, a_idx).squeeze(1), y, delta=1.0)
    n = width // 3
    logits = z[:, :3 * n].view(-1, 3, n).gather(1, a_idx.unsqueeze(2).expand(-1, 1, n)).squeeze(1)
    return -(dist[:, :n] * torch.log_softmax(logits, dim=1)).sum(dim=1).mean()


def head(args):
    B = args.batch
    widths = [int(w) for w in args.widths.split(",")]
    env, rb = played_env(256, 40, rb=20_000)
    lay = "nhwc_slot"
    idx = rb.sample_indices(B, seed=3, update_idx=0)
    a = rb.batch(idx, layout=lay, fields=("actions",)).actions
    a_idx = a.long().unsqueeze(1)
    y = torch.randn(B, device=DEV)
    dist = torch.softmax(torch.randn(B, max(widths) // 3 + 1, device=DEV), dim=1)
    plain = QT.TorchQNet("f32", env=env, reserve=B)

    def no_head():   # `grad`'s update
        q = plain(replay=rb, indices=idx, layout=lay)
        torch.nn.functional.huber_loss(q.gather(1, a_idx).squeeze(1), y, delta=1.0).backward()
        plain.step()

    nets = {}
    for w in widths:
        nets[w] = QT.TorchQNet("f32", env=env, reserve=B)
        nets[w].attach_head(w, seed=w)

    def with_head(w):
        net = nets[w]

        def run():
            q, z = net.forward(replay=rb, indices=idx, layout=lay, head=True)
            head_loss(w, q, z, a_idx, y, dist).backward()
            net.step()
        return run

    if args.kernels:   # for rocprofv3 --kernel-trace --stats: the same launches, untimed
        for _ in range(args.kernels):
            no_head()
            for w in widths:
                with_head(w)()
    else:
        base = time_device(no_head, args.reps, args.warmup)
        print(f"wide head, B = {B}, f32 (forward + loss in torch + backward + step):")
        print(f"  {'no head (grad)':24s} {fmt(base)}")
        for w in widths:
            us = time_device(with_head(w), args.reps, args.warmup)
            print(f"  {'width ' + str(w):24s} {fmt(us)}   + {statistics.median(us) - statistics.median(base):.1f} us")
    for net in [plain] + list(nets.values()):
        net.sync()
    env.close()


def time_alternated(fns, reps, warmup):
    """time_device for several paths, one call of each in turn, so that a drift of the clocks meets all of them alike"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return out


def torch_dist_loss(kind, N, z, z_next, b, rows, atoms, v_min, v_max):
    """the example's losses (scripts/torch_qrdqn_example.py): a*, the target and the loss of the taken action, in torch"""
    live = b.discounts * (1.0 - b.terminals.float())
    zn = z_next.view(-1, 3, N)
    taken = z.view(-1, 3, N)[rows, b.actions.long()]
    if kind == "quantile":
        nxt = zn[rows, zn.mean(dim=2).argmax(dim=1)]
        u = (b.returns[:, None] + live[:, None] * nxt)[:, None, :] - taken[:, :, None]
        huber = torch.where(u.abs() <= 1, 0.5 * u * u, u.abs() - 0.5)
        tau = (torch.arange(N, device=z.device, dtype=z.dtype) + 0.5) / N
        return ((tau[None, :, None] - (u.detach() < 0).float()).abs() * huber).mean(dim=2).sum(dim=1).mean()
    p = torch.softmax(zn, dim=2)
    nxt = p[rows, (p * atoms).sum(dim=2).argmax(dim=1)]
    delta = (v_max - v_min) / (N - 1)
    tz = (b.returns[:, None] + live[:, None] * atoms[None, :]).clamp(v_min, v_max)
    hat = (1.0 - (tz[:, None, :] - atoms[None, :, None]).abs() / delta).clamp(min=0.0)
    m = (nxt[:, None, :] * hat).sum(dim=2)
    return -(m * torch.log_softmax(taken, dim=1)).sum(dim=1).mean()


def dist(args):
    if not torch.cuda.is_available():
        sys.exit("torch_qnet_bench.py dist: no GPU")
    B = args.batch
    env, rb = played_env(256, 40, rb=20_000)
    lay = "nhwc_slot"
    idx = rb.sample_indices(B, seed=3, update_idx=0)
    b = rb.batch(idx, n_step=3, gamma=0.99, layout=lay, fields=("actions", "returns", "discounts", "terminals", "last_indices"))
    rows = torch.arange(B, device=DEV)
    a_idx = b.actions.long().unsqueeze(1)
    y = torch.randn(B, device=DEV)
    v_min, v_max = -10.0, 10.0
    plain = QT.TorchQNet("f32", env=env, reserve=B)

    def no_head():   # `grad`'s update
        q = plain(replay=rb, indices=idx, layout=lay)
        torch.nn.functional.huber_loss(q.gather(1, a_idx).squeeze(1), y, delta=1.0).backward()
        plain.step()

    cases, nets = [], [plain]
    for kind, N in (("quantile", 51), ("quantile", 200), ("categorical", 51)):
        d = QT.Quantile(N) if kind == "quantile" else QT.Categorical(N, v_min, v_max)
        atoms = torch.linspace(v_min, v_max, N, device=DEV)
        z_next = torch.randn(B, 3 * N, device=DEV)
        by_torch, fused = QT.TorchQNet("f32", env=env, reserve=B), QT.TorchQNet("f32", env=env, reserve=B)
        by_torch.attach_head(3 * N, seed=N)
        fused.attach_head(3 * N, seed=N)
        nets += [by_torch, fused]

        def torch_path(net=by_torch, kind=kind, N=N, z_next=z_next, atoms=atoms):
            _, z = net.forward(replay=rb, indices=idx, layout=lay, head=True)
            torch_dist_loss(kind, N, z, z_next, b, rows, atoms, v_min, v_max).backward()
            net.step()

        def fused_path(net=fused, d=d, z_next=z_next):
            net.train_dist(d, b.actions, b.returns, b.discounts, b.terminals, z_next, replay=rb, indices=idx, layout=lay)

        def values_path(net=fused, d=d, z_next=z_next):
            net.head_values(z_next, d, want="actions")

        cases.append((f"{kind} N = {N}", torch_path, fused_path, values_path))

    if args.kernels:   # for rocprofv3 --kernel-trace --stats: the same launches, untimed
        for _ in range(args.kernels):
            no_head()
            for _, torch_path, fused_path, values_path in cases:
                torch_path()
                fused_path()
                values_path()
    else:
        base = time_device(no_head, args.reps, args.warmup)
        mb = statistics.median(base)
        print(f"distributional update, B = {B}, f32, off the replay ring (median [min..max] of {args.reps} after {args.warmup}):")
        print(f"  {'no head (grad)':38s} {fmt(base)}")
        for name, torch_path, fused_path, values_path in cases:
            t, f = time_alternated((torch_path, fused_path), args.reps, args.warmup)
            print(f"  {name + ', loss in torch':38s} {fmt(t)}   + {statistics.median(t) - mb:.1f} us")
            print(f"  {name + ', train_dist':38s} {fmt(f)}   + {statistics.median(f) - mb:.1f} us")
    for net in nets:
        net.sync()
    env.close()


def head_act(args):
    if not torch.cuda.is_available():
        sys.exit("torch_qnet_bench.py head_act: no GPU")
    N, eps = 51, 0.1
    print(f"acting with a 3 x {N} head, f32, epsilon {eps}, on the env's ring (median [min..max] of {args.reps} after {args.warmup}):")
    for n in (int(x) for x in args.ns.split(",")):
        env, _ = played_env(n, 5)
        lay = "nchw_time"
        for d in (QT.Quantile(N), QT.Categorical(N, -10.0, 10.0)):
            net = QT.TorchQNet("f32", env=env, reserve=n)
            net.attach_head(3 * N, seed=N)
            step = [0]

            def three_calls(net=net, d=d):
                with torch.no_grad():
                    _, z = net.forward(env=env, layout=lay, head=True)
                    greedy = net.head_values(z, d, want="actions")
                explore = torch.rand(n, device=DEV) < eps
                return torch.where(explore, torch.randint(0, 3, (n,), device=DEV, dtype=torch.uint8), greedy)

            def one_call(net=net, d=d):
                step[0] += 1
                return net.act(d, eps, 7, step[0], env=env, layout=lay)

            t, f = time_alternated((three_calls, one_call), args.reps, args.warmup)
            name = type(d).__name__.lower()
            print(f"  n = {n:5d} {name + ', forward + head_values + torch mix':48s} {fmt(t)}")
            print(f"  n = {n:5d} {name + ', act()':48s} {fmt(f)}   {statistics.median(t) - statistics.median(f):+.1f} us saved")
            net.sync()
        env.close()


def pack(args):
    n = args.n
    net = QT.TorchQNet("bf16", reserve=n)
    x = torch.randint(0, 256, (n, 84, 84, 4), device=DEV, dtype=torch.uint8)
    x_host = x.cpu().numpy()
    for _ in range(args.reps):
        net.q(x, layout="nhwc_slot", want="actions")                       # k_pack_states<NHWC_SLOT>
        net.q(x.view(n, 4, 84, 84), layout="nchw_time", want="actions")     # k_pack_states<NCHW_TIME> (any bytes do)
    net.sync()
    for _ in range(max(2, args.reps // 4)):
        net.model.q_values(x_host)                                         # k_pack_obs
    print(f"pack: n = {n}, {2 * 28224 * n} bytes read + written per launch; kernel times are the trace's")
    net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("act", "update", "grad", "head", "dist", "head_act", "pack"))
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--arch", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--reps", type=int, default=None, help="default 20, dist: 30")
    ap.add_argument("--warmup", type=int, default=None, help="default 3, dist: 5")
    ap.add_argument("--widths", default="4,153,600", help="head: the head widths, comma separated")
    ap.add_argument("--ns", default="256,8192", help="head_act: the env counts, comma separated")
    ap.add_argument("--kernels", type=int, default=0, help="grad, head, dist: run this many of each path untimed (kernel trace)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 30 if args.what in ("dist", "head_act") else 20
    if args.warmup is None:
        args.warmup = 5 if args.what in ("dist", "head_act") else 3
    {"act": act, "update": update, "grad": grad, "head": head, "dist": dist, "head_act": head_act, "pack": pack}[args.what](args)


if __name__ == "__main__":
    np.random.seed(0)
    main()
