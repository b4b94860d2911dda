"""Float64 torch reference of the GPU Q-network's *mixed-precision contract* (test infrastructure).

The product computes the Nature-DQN with bf16 MFMA operands and fp32 accumulation.  Its storage points
are: bf16 copies of the conv1..conv3 / full_layer kernels (fp32 master kept), bf16 post-ReLU activations
a1..a4, bf16 activation gradients dz1..dz4; the action layer, biases, Huber and Adam stay fp32.  This
module reproduces exactly those rounding points (round-to-nearest-even, like v_cvt_pk_bf16_f32) and
computes everything else in float64, so the GPU kernels can be checked tightly (only accumulation
order differs), independently of the bf16-vs-fp32 precision gap that the fp32 oracle comparison states.

Teacher forcing (forward_backward_full(acts=...)): every layer's emulated output is computed from the product's own
stored activation of the layer below, and the backward uses the product's activations as ReLU masks and as the
weight gradients' inputs; with q=... the loss gradient is taken at the product's own Q.  The emulation and the product
then differ by one layer's accumulation order plus isolated bf16 rounding flips (of the stored dz3..dz1 in the
backward, which the product does not expose); nothing compounds through Q and the Huber kink.
"""
import numpy as np
import torch


def bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundBoth(torch.autograd.Function):
    """Rounds the value and the incoming gradient to bf16 (stored activation and activation grad)."""

    @staticmethod
    def forward(ctx, x):
        return bf16(x)

    @staticmethod
    def backward(ctx, g):
        return bf16(g)


class _Forced(torch.autograd.Function):
    """A stored activation replaced by the product's own: the value is `given`, the incoming gradient is rounded to
    bf16 (the stored dz) and masked by given > 0 (the product's ReLU mask), then flows into the emulated pre-activation."""

    @staticmethod
    def forward(ctx, z, given):
        ctx.save_for_backward(given > 0)
        return given.clone()

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return bf16(g) * mask, None


def forward_backward_full(weights, x_u8, actions=None, y=None, acts=None, q=None, dtype=torch.float64):
    """The contract in `dtype` accumulation.  acts: the product's stored a1..a4 (qlx_model_last_activation; a1..a3 as
    [B][H][W][C] or flat, a4 [B][512]) for teacher forcing, or None.  q: the product's own Q [B][3] (with acts, actions and
    y): the head is then restated as the product computes it, in float32 from that Q - e = q_a - y, dloss/dq_a =
    clip(e, -1, 1) / B, dz4 = bf16(float32(dloss/dq_a * W4[k][a])) (a4 > 0) - and handed to the dense backward.  (Without it
    the ~1e-6 accumulation noise of Q moves dloss/dq of a sample with a small error by ~1e-5, and even at the product's Q a
    float64 head differs from the float32 one by ~1e-7: either flips bf16 roundings of that sample's dz4 row, and each flip
    perturbs all 3136 dz3 elements of the sample - at small B up to several 1e-3 of the conv gradients.)  Returns a dict:
      q     [B][3]        Q emulated from the (forced) a4
      acts  4 arrays      each layer's emulated stored activation, NHWC / [B][512], computed from the layer input in use
      S     4 arrays      sum |a||w| + |b| of each activation element (the same conv / matmul on absolute values)
      loss, grads         when actions / y are given (grads in the Keras layouts)"""
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
    ws = [t(w) for w in weights]
    for i in (0, 2, 4, 6):
        ws[i] = bf16(ws[i])
    params = [w.clone().requires_grad_(True) for w in ws]
    k0, b0, k1, b1, k2, b2, k3, b3, k4, b4 = params
    R = _RoundBoth.apply
    B = np.asarray(x_u8).shape[0]
    shapes = [(B, 20, 20, 32), (B, 9, 9, 64), (B, 7, 7, 64), (B, 512)]
    given = [None] * 4 if acts is None else [t(np.asarray(a).reshape(s)) for a, s in zip(acts, shapes)]
    nchw = lambda a: a.permute(0, 3, 1, 2)
    conv = torch.nn.functional.conv2d
    emu, S, pre = [], [], []

    def layer(h_in, k, b, stride, l):
        if k.dim() == 4:
            z = conv(h_in, k.permute(3, 2, 0, 1), b, stride=stride)
            with torch.no_grad():
                S.append(conv(h_in.abs(), k.abs().permute(3, 2, 0, 1), b.abs(), stride=stride).permute(0, 2, 3, 1).numpy())
        else:
            z = h_in @ k + b
            with torch.no_grad():
                S.append((h_in.abs() @ k.abs() + b.abs()).numpy())
        if given[l] is None:
            h = R(torch.relu(z))
            emu.append((h.permute(0, 2, 3, 1) if h.dim() == 4 else h).detach().numpy())
            return h
        pre.append(z)
        with torch.no_grad():
            e = bf16(torch.relu(z))
            emu.append((e.permute(0, 2, 3, 1) if e.dim() == 4 else e).numpy())
        return _Forced.apply(z, nchw(given[l]) if z.dim() == 4 else given[l])

    h = layer(nchw(t(x_u8)), k0, b0, 4, 0)
    h = layer(h, k1, b1, 2, 1)
    h = layer(h, k2, b2, 1, 2)
    h = layer(h.permute(0, 2, 3, 1).reshape(B, -1), k3, b3, 1, 3)
    q_given, q = q, (h if q is None else h.detach()) @ k4 + b4
    out = dict(q=q.detach().numpy(), acts=emu, S=S)
    if actions is None:
        return out
    act = np.asarray(actions, dtype=np.int64)
    if q_given is None:
        qa = q[torch.arange(B), torch.as_tensor(act)]
        loss = torch.nn.functional.huber_loss(qa, t(y), delta=1.0, reduction="mean")
        loss.backward()
        out["loss"] = loss.item()
    else:   # the head in float32 as k_fc2_train computes it, from the product's Q
        f, ar = np.float32, np.arange(B)
        e = np.asarray(q_given, f)[ar, act] - np.asarray(y, f)
        g = np.clip(e, f(-1.0), f(1.0)) / f(B)
        dz4 = g[:, None] * np.asarray(weights[8], f)[:, act].T
        assert e.dtype == g.dtype == dz4.dtype == f
        gq = np.zeros((B, 3))
        gq[ar, act] = g
        e = e.astype(np.float64)
        out["loss"] = (t(np.where(np.abs(e) <= 1.0, 0.5 * e * e, np.abs(e) - 0.5)).sum() / B).item()
        torch.autograd.backward([q, pre[3]], [t(gq), bf16(t(dz4)) * (given[3] > 0)])
    out["grads"] = [p.grad.numpy() for p in params]
    return out


def forward_backward(weights, x_u8, actions=None, y=None):
    """Returns q (float64 numpy) and, when actions/y are given, (loss, grads list in Keras layouts)."""
    r = forward_backward_full(weights, x_u8, actions, y)
    if actions is None:
        return r["q"]
    return r["q"], r["loss"], r["grads"]
