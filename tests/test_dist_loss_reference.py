"""The restatements of tests/dist_loss_reference.py held to independent statements, without a GPU: the float64 quantile loss
against the example's quantile_huber in float64 torch (value and autograd gradient), the gather form of the C51 projection
against the classic floor / ceil scatter, the categorical gradient against autograd, and the float32 quantile restatement
against the float64 one."""
import ast
import os

import numpy as np
import pytest
import torch

import dist_loss_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def example_quantile_huber():
    """quantile_huber of scripts/torch_qrdqn_example.py, taken from its source (importing the script would open the library)"""
    tree = ast.parse(open(os.path.join(ROOT, "scripts", "torch_qrdqn_example.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "quantile_huber"]
    assert len(fn) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "quantile_huber", "exec"), ns)
    return ns["quantile_huber"]


def batch(rng, B, N, scale=1.5):
    return dict(z=(scale * rng.normal(size=(B, 3 * N))).astype(np.float32),
                actions=rng.integers(0, 3, B).astype(np.uint8),
                returns=rng.normal(size=B).astype(np.float32),
                discounts=np.full(B, 0.99 ** 3, np.float32),
                terminals=(rng.random(B) < 0.2).astype(np.uint8),
                z_next=(scale * rng.normal(size=(B, 3 * N))).astype(np.float32))


@pytest.mark.parametrize("N", [1, 2, 51, 65])
def test_quantile64_is_the_examples_loss_and_its_gradient(N):
    rng = np.random.default_rng(N)
    B = 7
    b = batch(rng, B, N)
    ref = R.quantile64(N=N, **b)
    qh = example_quantile_huber()
    z = torch.tensor(b["z"], dtype=torch.float64, requires_grad=True)
    zn = torch.tensor(b["z_next"], dtype=torch.float64).view(B, 3, N)
    a_star = zn.mean(dim=2).argmax(dim=1)
    assert np.array_equal(a_star.numpy(), ref["a_star"])
    live = torch.tensor(b["discounts"], dtype=torch.float64) * (1.0 - torch.tensor(b["terminals"], dtype=torch.float64))
    y = torch.tensor(b["returns"], dtype=torch.float64)[:, None] + live[:, None] * zn[torch.arange(B), a_star]
    loss = qh(z.view(B, 3, N)[torch.arange(B), torch.tensor(b["actions"].astype(np.int64))], y)
    loss.backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-13 * max(1.0, abs(ref["loss"]))
    assert np.abs(z.grad.numpy() - ref["dz"]).max() <= 1e-14
    assert np.abs(ref["dz"]).max() > 0
    # weights scale a sample's loss and gradient; a caller's a* is used as given
    w = rng.random(B).astype(np.float32) + 0.5
    other = ((ref["a_star"] + 1) % 3).astype(np.uint8)
    rw = R.quantile64(N=N, weights=w, a_star=other, **b)
    one = [R.quantile64(N=N, a_star=other[i:i + 1], **{k: v[i:i + 1] for k, v in b.items()}) for i in range(B)]
    assert np.allclose(rw["loss"], sum(float(w[i]) * one[i]["loss"] for i in range(B)) / B, rtol=1e-13)
    assert np.allclose(rw["dz"], np.concatenate([float(w[i]) * one[i]["dz"] for i in range(B)]) / B, rtol=1e-13, atol=0)


def c51_case(rng, B, N, v_min, v_max):
    b = batch(rng, B, N, scale=1.0)
    zk, delta = R.atoms64(N, v_min, v_max)
    span = v_max - v_min
    b["returns"] = (v_min + span * rng.random(B)).astype(np.float32)
    # directed rows: a return exactly on an atom with nothing bootstrapped, clipped at both ends, live = 0
    b["terminals"][:4] = [1, 0, 0, 1]
    b["returns"][0] = np.float32(zk[N // 2]) if float(np.float32(zk[N // 2])) == zk[N // 2] else np.float32(zk[0])
    b["returns"][1] = np.float32(v_max + 3 * span)
    b["returns"][2] = np.float32(v_min - 3 * span)
    b["returns"][3] = np.float32(v_min + 0.3 * span)
    return b, zk, delta


@pytest.mark.parametrize("v_min,v_max", [(-10.0, 10.0), (0.0, 1.0)])
@pytest.mark.parametrize("N", [2, 3, 51, 64, 65, 341])
def test_gather_projection_is_the_scatter_projection(N, v_min, v_max):
    rng = np.random.default_rng(100 + N)
    B = 8
    b, zk, delta = c51_case(rng, B, N, v_min, v_max)
    ref = R.categorical64(N=N, v_min=v_min, v_max=v_max, **b)
    zn = R.f64(b["z_next"]).reshape(B, 3, N)[np.arange(B), ref["a_star"].astype(np.int64)]
    e = np.exp(zn - zn.max(axis=1, keepdims=True))
    pn = e / e.sum(axis=1, keepdims=True)
    live = np.where(b["terminals"] != 0, 0.0, R.f64(b["discounts"]))
    Tz = np.clip(R.f64(b["returns"])[:, None] + live[:, None] * zk[None, :], zk[0], zk[-1])
    gather = R.project_gather(pn, Tz, zk, delta)
    scatter = R.project_scatter(pn, Tz, N, zk[0], delta)
    assert np.abs(gather - ref["m"]).max() <= 1e-15
    assert np.abs(gather - scatter).max() <= 1e-12, float(np.abs(gather - scatter).max())
    assert np.abs(gather.sum(axis=1) - 1.0).max() <= 1e-12
    # the directed rows: all mass on one atom
    on_atom = int(np.argmin(np.abs(zk - float(b["returns"][0]))))
    if zk[on_atom] == float(b["returns"][0]):
        assert abs(gather[0, on_atom] - 1.0) <= 1e-12
    assert abs(gather[1, N - 1] - 1.0) <= 1e-12 and abs(gather[2, 0] - 1.0) <= 1e-12
    assert (gather[3] > 1e-9).sum() <= 2 and abs(gather[3].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("N", [2, 51, 65])
def test_categorical64_gradient_is_autograds(N):
    rng = np.random.default_rng(200 + N)
    B, v_min, v_max = 6, -10.0, 10.0
    b, zk, delta = c51_case(rng, B, N, v_min, v_max)
    w = rng.random(B).astype(np.float32) + 0.5
    ref = R.categorical64(N=N, v_min=v_min, v_max=v_max, weights=w, **b)
    z = torch.tensor(b["z"], dtype=torch.float64, requires_grad=True)
    taken = z.view(B, 3, N)[torch.arange(B), torch.tensor(b["actions"].astype(np.int64))]
    Lb = -(torch.tensor(ref["m"]) * torch.log_softmax(taken, dim=1)).sum(dim=1)
    loss = (torch.tensor(w, dtype=torch.float64) * Lb).mean()
    loss.backward()
    assert np.abs(Lb.detach().numpy() - ref["sample_loss"]).max() <= 1e-12
    assert abs(loss.item() - ref["loss"]) <= 1e-12
    assert np.abs(z.grad.numpy() - ref["dz"]).max() <= 1e-14
    assert np.abs(ref["dz"]).max() > 0
    # values: the expectation under the softmax
    q, a, mq = R.values64_categorical(b["z"], N, v_min, v_max)
    want = (torch.softmax(torch.tensor(b["z"], dtype=torch.float64).view(B, 3, N), dim=2) * torch.tensor(zk)).sum(dim=2).numpy()
    assert np.abs(q - want).max() <= 1e-12 and np.array_equal(a, want.argmax(axis=1)) and np.array_equal(mq, q.max(axis=1))


@pytest.mark.parametrize("N", [1, 2, 3, 17, 51, 64, 65, 128, 200, 256, 257, 341])
def test_quantile32_is_within_gamma_of_quantile64(N):
    """gamma(N + 4) times the sum of the absolute terms: a chain over j is N - 1 additions of terms that carry four
    roundings (T's two, u's, the product's).  A term's magnitude is taken before the cancellation in u = T - theta:
    omega (|returns| + |live z_next_j| + |theta_i|) for omega clamp(u), and 0.5 more for omega h (|h| <= |u| + 0.5 and
    |dh/du| <= 1, so u's rounding error reaches h no larger than it reaches u).  L_b and the loss sum such rows."""
    rng = np.random.default_rng(300 + N)
    B = 9
    b = batch(rng, B, N)
    w = rng.random(B).astype(np.float32) + 0.5
    r32 = R.quantile32(N=N, weights=w, **b)
    r64 = R.quantile64(N=N, weights=w, **b)
    assert np.array_equal(r32["a_star"], r64["a_star"])
    rows, act = np.arange(B), b["actions"].astype(np.int64)
    z = R.f64(b["z"]).reshape(B, 3, N)[rows, act]
    zn = R.f64(b["z_next"]).reshape(B, 3, N)[rows, r64["a_star"].astype(np.int64)]
    live = np.where(b["terminals"] != 0, 0.0, R.f64(b["discounts"]))
    ret = R.f64(b["returns"])
    u = (ret[:, None] + live[:, None] * zn)[:, None, :] - z[:, :, None]
    tau = (np.arange(N) + 0.5) / N
    om = np.abs(tau[None, :, None] - (u < 0))
    mag = (np.abs(ret)[:, None] + np.abs(live[:, None] * zn))[:, None, :] + np.abs(z)[:, :, None]
    g = R.gamma(N + 4)
    wd = R.f64(w)
    bound_dz = g * (om * mag).sum(axis=2) / N * wd[:, None] / B
    bound_l = g * (om * (mag + 0.5)).sum(axis=(1, 2)) / N
    bound_loss = float((wd * bound_l).sum() / B)
    err_dz = np.abs(R.f64(r32["dz"]) - r64["dz"]).reshape(B, 3, N)[rows, act]
    err_l = np.abs(R.f64(r32["sample_loss"]) - r64["sample_loss"])
    ratios = (float((err_dz / bound_dz).max()), float((err_l / bound_l).max()), abs(float(r32["loss"]) - r64["loss"]) / bound_loss)
    print(f"N {N}: float32 against float64, max err / bound: dz {ratios[0]:.3g}, L_b {ratios[1]:.3g}, loss {ratios[2]:.3g}")
    assert max(ratios) <= 1.0
    assert np.abs(r64["dz"]).max() > 0 and not r32["dz"].reshape(B, 3, N)[rows, (act + 1) % 3].any()
    # both Huber branches and both signs of u occur
    assert (np.abs(u) <= 1).any() and (np.abs(u) > 1).any() and (u < 0).any() and (u > 0).any()
