"""The batched Breakout env, the HBM replay, its sampler and the Q-net for an agent that lives in PyTorch device tensors.

Everything here is plumbing over libqlx's device-pointer calls (include/qlx.h "Device-tensor env and replay calls",
"Q-network on device tensors" and "Prioritized replay on device tensors"): observations, steps,
pushes, sampled n-step batches, prioritized draws and priority writes, Q-values, whole updates and the gradients of a
loss written in torch go from kernel to tensor without touching the host.  No call synchronises; order against torch's work is
kept by stream waits (below).

One HIP runtime per process.  torch's wheel carries a libamdhip64 of its own, libqlx.so asks for the system's by
SONAME.  With torch loaded first the loader gives libqlx torch's copy, and a pointer or stream of one is the other's;
with libqlx loaded first the process holds two runtimes, and is of no use here.  So this module imports torch, then
loads libqlx, then checks /proc/self/maps: import qlx_torch before any other use of qlx.

Streams.  Each object runs on its own HIP stream (a TorchReplay made from an env shares the env's).  Every call makes
that stream wait for torch's current stream, enqueues, and makes the current stream wait for it, so tensors computed by
torch just before a call are complete when the kernel reads them, and results can be used by torch at once: a call
behaves like a torch op on the current stream.  Tensors handed in or out are record_stream'ed on that current stream,
which the wait has put behind the kernel, and never on the object's own stream: torch's allocator records an event on
every recorded stream when such a tensor is freed, which may be after close() has destroyed the object's stream.

Dtypes: states, actions, terminals, dones and masks are uint8; rewards, returns and discounts float32; indices and
last_indices are int64 holding the ABI's uint64 (a negative value reads as an index >= len), steps int32 (uint32).
"""
import collections
import contextlib
import ctypes as C
import math
import os
import weakref

import torch

import qlx
from qlx import OBS_NCHW_TIME, OBS_NHWC_SLOT, QlError

_L = qlx.lib()


def mapped_hip_runtimes():
    """paths of the libamdhip64 images mapped into this process"""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split(None, 5)
            if len(parts) == 6 and os.path.basename(parts[5].strip()).startswith("libamdhip64.so"):
                paths.add(parts[5].strip())
    return sorted(paths)


def _check_one_runtime():
    rts = mapped_hip_runtimes()
    if len(rts) != 1:
        raise QlError("qlx_torch must be imported before any other use of qlx: this process maps "
                      f"{len(rts)} HIP runtimes ({', '.join(rts) or 'none'}), so torch and libqlx cannot share "
                      "pointers and streams")


_check_one_runtime()

MAX_BATCH = 4096
_LAYOUTS = {"nhwc_slot": OBS_NHWC_SLOT, "nchw_time": OBS_NCHW_TIME}
_STATE_SHAPE = {OBS_NHWC_SLOT: (qlx.FRAME, qlx.FRAME, qlx.SLOTS), OBS_NCHW_TIME: (qlx.SLOTS, qlx.FRAME, qlx.FRAME)}

_FIELDS = ("s", "s_next", "actions", "returns", "discounts", "terminals", "last_indices", "steps")   # qlx_batch_dev
_BATCH_DTYPES = dict(actions=torch.uint8, returns=torch.float32, discounts=torch.float32, terminals=torch.uint8,
                     last_indices=torch.int64, steps=torch.int32)


class Batch(collections.namedtuple("Batch", "s s_next actions returns discounts terminals indices steps")):
    """(s, s_next, actions, returns, discounts, terminals, indices, steps); `indices` are the transitions asked for or
    drawn, and the attribute `last_indices` holds each n-step window's last transition (the one s_next belongs to)"""
    last_indices = None


def _layout(layout):
    try:
        return _LAYOUTS[layout]
    except (KeyError, TypeError):
        raise ValueError(f"layout must be 'nchw_time' or 'nhwc_slot', not {layout!r}") from None


def _device(device):
    d = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
    if d.type != "cuda":
        raise ValueError(f"device must be a CUDA (HIP) device, not {d}")
    return torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)


def _arg(name, t, device, dtype, shape):
    """`t` as the kernels need it, or ValueError before anything is launched"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor")
    if not t.is_cuda or t.device != device:
        raise ValueError(f"{name} must be on {device}, not {t.device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned")
    return t


class _Streamed:
    """an object of libqlx with a HIP stream of its own, ordered against torch's current stream call by call"""

    def _wrap_stream(self, getter):
        p = C.c_void_p()
        qlx._check(getter(self.h, C.byref(p)))
        self.stream = torch.cuda.ExternalStream(p.value or 0, device=self.device)

    class _Ordered:
        def __init__(self, obj, tensors):
            self.obj, self.tensors = obj, tensors

        def __enter__(self):
            o = self.obj
            if o.h is None:
                raise QlError("the object is closed")
            self.current = torch.cuda.current_stream(o.device)
            o.stream.wait_stream(self.current)

        def __exit__(self, *exc):
            self.current.wait_stream(self.obj.stream)
            for t in self.tensors:
                if t is not None:
                    t.record_stream(self.current)   # a no-op for a tensor allocated on it, the usual case
            return False

    def _ordered(self, *tensors):
        return self._Ordered(self, tensors)


class TorchEnv(_Streamed):
    """n batched Breakout envs stepped with device tensors"""

    ACTION_SPACE = qlx.ACTION_SPACE

    def __init__(self, n_envs, seed=0x51A5EED, device="cuda:0"):
        self.device = _device(device)
        self._env = qlx.BreakoutEnvironment(n_envs, seed, self.device.index)
        self.h = self._env.h
        self.n = self._env.n
        self._wrap_stream(_L.qlx_env_stream)
        self._sharing = weakref.WeakSet()   # replays that run on this env's stream: closed before it
        self.writes = 0   # steps and resets so far: a TorchQNet backward checks that its forward's states still stand

    def close(self):
        for rb in list(getattr(self, "_sharing", ())):
            rb.close()
        env = getattr(self, "_env", None)
        if env is not None:
            env.close()
        self.h = None

    def obs(self, layout="nchw_time", out=None):
        """current states: uint8 [n, 4, 84, 84] (channel 0 oldest) or, 'nhwc_slot', [n, 84, 84, 4] (x, y, ring slot)"""
        lay = _layout(layout)
        shape = (self.n,) + _STATE_SHAPE[lay]
        out = torch.empty(shape, dtype=torch.uint8, device=self.device) if out is None else _arg("out", out, self.device, torch.uint8, shape)
        with self._ordered(out):
            qlx._check(_L.qlx_env_obs_dev(self.h, lay, out.data_ptr()))
        return out

    def step(self, actions):
        """one step of every env with uint8 actions [n] (values >= 3: action 0 and an error at sync()); (rewards, dones)"""
        a = _arg("actions", actions, self.device, torch.uint8, (self.n,))
        rewards = torch.empty(self.n, dtype=torch.float32, device=self.device)
        dones = torch.empty(self.n, dtype=torch.uint8, device=self.device)
        self.writes += 1
        with self._ordered(a, rewards, dones):
            qlx._check(_L.qlx_env_step_dev(self.h, a.data_ptr(), rewards.data_ptr(), dones.data_ptr()))
        return rewards, dones

    def reset(self, mask=None):
        """reset every env, or those with mask[i] != 0 (uint8 device tensor [n])"""
        m = None if mask is None else _arg("mask", mask, self.device, torch.uint8, (self.n,))
        self.writes += 1
        with self._ordered(m):
            qlx._check(_L.qlx_env_reset_dev(self.h, None if m is None else m.data_ptr()))

    def sync(self):
        """wait for the env's stream; QlError if a step met an action >= 3"""
        qlx._check(_L.qlx_env_sync(self.h))

    def mechanics(self):
        return self._env.mechanics()

    def hashes(self):
        return self._env.hashes()


class TorchReplay(_Streamed):
    """the HBM replay ring read into device tensors.  TorchReplay(capacity, env) makes a replay on the env's stream;
    TorchReplay(handle=h, n_envs=n, device=d) wraps a handle someone else owns (a learner's replay) on its own stream."""

    def __init__(self, capacity=0, env=None, handle=None, n_envs=None, device=None):
        if handle is None:
            if env is None:
                raise ValueError("TorchReplay needs an env (or a handle)")
            self.device = env.device
            self.n = env.n
            self._rb = qlx.ReplayBuffer(capacity, env.n, self.device.index)
            self._env = env   # the stream is the env's: keep it alive
            self.h = self._rb.h
            qlx._check(_L.qlx_replay_share_stream(self.h, env.h))
            env._sharing.add(self)
        else:
            if n_envs is None:
                raise ValueError("a wrapped replay handle needs n_envs")
            self.device = _device("cuda:0" if device is None else device)
            self.n = n_envs
            self._rb = qlx.ReplayBuffer(0, 0, handle=handle)
            self.h = handle
        self._wrap_stream(_L.qlx_replay_stream)
        self.writes = 0   # pushes through add() so far (see TorchEnv.writes)

    def close(self):
        rb = getattr(self, "_rb", None)
        if rb is not None:
            rb.close()
        self.h = None

    def __len__(self):
        return len(self._rb)

    def add(self, env, actions, rewards, dones):
        """the transition every env just made: the actions given to env.step and what it returned"""
        if env.n != self.n or env.device != self.device:
            raise ValueError("env does not match the replay (n_envs, device)")
        a = _arg("actions", actions, self.device, torch.uint8, (self.n,))
        r = _arg("rewards", rewards, self.device, torch.float32, (self.n,))
        d = _arg("dones", dones, self.device, torch.uint8, (self.n,))
        self.writes += 1
        # the push runs on the env's stream (it reads the env's ring); with a shared stream the two are one
        with env._ordered(a, r, d), self._ordered(a, r, d):
            qlx._check(_L.qlx_replay_push_dev(self.h, env.h, a.data_ptr(), r.data_ptr(), d.data_ptr()))

    def sample_indices(self, batch, seed, update_idx, rank=0):
        """`batch` distinct logical indices < len from stream (seed, update_idx, rank), int64 [batch]"""
        if not 0 < batch <= MAX_BATCH:
            raise ValueError(f"batch must be in 1..{MAX_BATCH}")
        if batch > len(self):
            raise ValueError(f"batch {batch} > len {len(self)}")
        idx = torch.empty(batch, dtype=torch.int64, device=self.device)
        with self._ordered(idx):
            qlx._check(_L.qlx_replay_sample_distinct_dev(self.h, seed, update_idx, rank, batch, idx.data_ptr()))
        return idx

    def batch(self, indices, n_step=1, gamma=0.99, layout="nchw_time", out=None, fields=None):
        """The transitions at `indices` (int64 [B]) as a Batch: s, s_next (the state after the n-step window's last
        transition), actions, returns = sum_{j<m} gamma^j r_j, discounts = gamma^m, terminals, indices (as given) and
        steps = m, with the windows' last indices as its attribute last_indices.  `fields`: the qlx_batch_dev names to
        produce (default all; the rest are None and cost nothing); `out`: a dict of tensors to write into, by those
        names.  An index >= len gives an all-zero sample and an error at sync()."""
        lay = _layout(layout)
        if not isinstance(indices, torch.Tensor) or indices.dim() != 1:
            raise ValueError("indices must be a 1-d tensor")
        B = indices.shape[0]
        if not 0 < B <= MAX_BATCH:
            raise ValueError(f"batch must be in 1..{MAX_BATCH}")
        if not 1 <= n_step <= 32:
            raise ValueError("n_step must be in 1..32")
        idx = _arg("indices", indices, self.device, torch.int64, (B,))
        out = dict(out or {})
        names = _FIELDS if fields is None else tuple(fields)
        unknown = (set(names) | set(out)) - set(_FIELDS)
        if unknown:
            raise ValueError(f"unknown batch fields {sorted(unknown)}")
        res = {}
        for k in _FIELDS:
            if k in ("s", "s_next"):
                dtype, shape = torch.uint8, (B,) + _STATE_SHAPE[lay]
            else:
                dtype, shape = _BATCH_DTYPES[k], (B,)
            if k in out:
                res[k] = _arg(f"out[{k!r}]", out[k], self.device, dtype, shape)
            elif k in names:
                res[k] = torch.empty(shape, dtype=dtype, device=self.device)
            else:
                res[k] = None
        o = qlx.BatchDev(**{k: (None if t is None else t.data_ptr()) for k, t in res.items()})
        with self._ordered(idx, *res.values()):
            qlx._check(_L.qlx_replay_batch_dev(self.h, idx.data_ptr(), B, n_step, gamma, lay, C.byref(o)))
        b = Batch(res["s"], res["s_next"], res["actions"], res["returns"], res["discounts"], res["terminals"], idx, res["steps"])
        b.last_indices = res["last_indices"]
        return b

    def sample(self, batch, seed, update_idx, n_step=1, gamma=0.99, layout="nchw_time", rank=0, out=None):
        """sample_indices + batch: `batch` distinct transitions drawn from stream (seed, update_idx, rank)"""
        return self.batch(self.sample_indices(batch, seed, update_idx, rank), n_step, gamma, layout, out)

    def enable_priorities(self):
        """Proportional prioritized replay from here on: the transitions held now get priority 1, later
        ones enter at the largest priority written so far.  Synchronises; a second call resets to that state."""
        if self.h is None:
            raise QlError("the object is closed")
        self._rb.per_enable()

    def sample_prioritized(self, batch, seed, update_idx, beta=0.4, rank=0):
        """`batch` draws (with replacement) in proportion to the priorities, from stream (seed, update_idx, rank):
        (indices int64 [batch], importance weights float32 [batch] = (len P(i))^-beta over the batch's largest)"""
        if not 0 < batch <= MAX_BATCH:
            raise ValueError(f"batch must be in 1..{MAX_BATCH}")
        idx = torch.empty(batch, dtype=torch.int64, device=self.device)
        w = torch.empty(batch, dtype=torch.float32, device=self.device)
        with self._ordered(idx, w):
            self._rb.per_sample_dev(seed, update_idx, batch, beta, idx.data_ptr(), w.data_ptr(), rank)
        return idx, w

    def update_priorities(self, indices, td_abs, alpha=0.6, eps=1e-6):
        """priority (td_abs + eps)^alpha for the transitions at `indices` (int64 [n], as they are now: before the next
        add on a full ring), td_abs float32 [n]; the last of a repeated index wins.  An index >= len or a td_abs that
        is NaN, infinite or negative writes nothing and gives an error at sync()."""
        if not isinstance(indices, torch.Tensor) or indices.dim() != 1:
            raise ValueError("indices must be a 1-d tensor")
        n = indices.shape[0]
        if n > MAX_BATCH:
            raise ValueError(f"at most {MAX_BATCH} priorities per call")
        idx = _arg("indices", indices, self.device, torch.int64, (n,))
        td = _arg("td_abs", td_abs, self.device, torch.float32, (n,))
        with self._ordered(idx, td):
            self._rb.per_update_dev(idx.data_ptr() or None, td.data_ptr() or None, n, alpha, eps)

    def priorities(self):
        """read-out (synchronises): dict of numpy leaves [capacity] by physical slot, tree [2L], total, per_max, start"""
        if self.h is None:
            raise QlError("the object is closed")
        return self._rb.per_get()

    def sync(self):
        """wait for the replay's stream; QlError, once, if a call since the last sync met an index >= len (or, with
        priorities, a td_abs that is NaN, infinite or negative)"""
        qlx._check(_L.qlx_replay_sync(self.h))


MAX_STATES = 8192
_ARCHS = {"f32": qlx.PREC_F32, "bf16": qlx.PREC_BF16}
_WHICH = {"s": 0, "s_next": 1}
_WANT = ("q", "actions", "max_q")


class _Pass:
    """one differentiable forward of a TorchQNet: its source, ticket and the write counts of what it read in place"""

    def __init__(self, src, n, ins, env, replay, ticket):
        self.src, self.n, self.ins, self.env, self.replay, self.ticket = src, n, ins, env, replay, ticket
        self.writes = [(o, o.writes) for o in (env, replay) if o is not None]


class _QFunction(torch.autograd.Function):
    """q = Q(states) with the backward through the net's HIP kernels.  The states are bytes, so the graph hangs on `anchor`,
    a scalar the net owns; the gradients go to the net's gradient buffer (TorchQNet.grads), not to a tensor."""

    @staticmethod
    def forward(ctx, anchor, net, source):
        ctx.net = net
        q, ctx.rec = net._forward_pass(*source)
        return q

    @staticmethod
    def backward(ctx, grad_q):
        ctx.net._backward_pass(ctx.rec, grad_q)
        return None, None, None


class _QZFunction(torch.autograd.Function):
    """(q, z) = (Q(states), the attached wide head's Z(states)) from one trunk forward, with one backward through the net's
    kernels for both: a missing grad for q passes no dq at all, a missing grad for z passes zeros."""

    @staticmethod
    def forward(ctx, anchor, net, source):
        ctx.net = net
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None, not as zeros
        q, z, ctx.rec = net._forward_pass_head(*source)
        return q, z

    @staticmethod
    def backward(ctx, grad_q, grad_z):
        ctx.net._backward_pass(ctx.rec, grad_q, grad_z, head=True)
        return None, None, None


class _Dist:
    """how a head of width 3 * atoms is read by the distributional calls (qlx_dist)"""

    def __init__(self, kind, atoms, v_min=0.0, v_max=0.0):
        self.atoms, self.width = int(atoms), 3 * int(atoms)
        self.c = qlx.Dist(kind, self.atoms, v_min, v_max)


class Quantile(_Dist):
    """Z[b][a * atoms + i] is quantile i of action a (QR-DQN): Q is the mean of the quantiles, the loss the quantile Huber
    loss with kappa = 1 and tau_i = (i + 0.5) / atoms"""

    def __init__(self, atoms):
        if not 1 <= int(atoms) <= qlx.DIST_MAX_ATOMS:
            raise ValueError(f"atoms must be in 1..{qlx.DIST_MAX_ATOMS}")
        super().__init__(qlx.DIST_QUANTILE, atoms)


class Categorical(_Dist):
    """Z[b][a * atoms + i] is the logit of atom z_i = v_min + i (v_max - v_min) / (atoms - 1) of action a (C51): Q is the
    expectation under the softmax, the loss the cross-entropy against the projected target distribution"""

    def __init__(self, atoms, v_min, v_max):
        if not 2 <= int(atoms) <= qlx.DIST_MAX_ATOMS:
            raise ValueError(f"atoms must be in 2..{qlx.DIST_MAX_ATOMS}")
        if not (math.isfinite(v_min) and math.isfinite(v_max) and v_min < v_max):
            raise ValueError("v_min and v_max must be finite with v_min < v_max")
        super().__init__(qlx.DIST_CATEGORICAL, atoms, v_min, v_max)
        self.v_min, self.v_max = float(v_min), float(v_max)


class _DistLossFunction(torch.autograd.Function):
    """loss = the distributional loss of z (TorchQNet.dist_loss); its backward hands dz * grad_loss on to z's grad_fn"""

    @staticmethod
    def forward(ctx, z, net, dist, args):
        loss, dz, sample_loss, a_star = net._dist_loss(z, dist, *args)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(dz, sample_loss, a_star)
        return loss, dz, sample_loss, a_star

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        (dz,) = ctx.saved_tensors
        return dz * grad_loss, None, None, None


class _DeviceFloats:
    """a device float32 array of libqlx as torch.as_tensor reads it (zero copy); keeps its owner alive"""

    def __init__(self, ptr, count, owner):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=(count,), typestr="<f4", data=(ptr, False), version=2, strides=None)


class TorchQNet(_Streamed):
    """The Nature-DQN Q-net (fp32 or bf16 kernels) on device tensors (include/qlx.h "Q-network on device tensors",
    DESIGN.md §16): Q-values of, and one whole update (forward, Huber, backward, clip, Adam) on, states that are dense
    tensors, transitions of a TorchReplay given by their indices, or a TorchEnv's current states, with targets computed in
    torch.  TorchQNet(env=env) runs on the env's stream and is closed with it; otherwise it has a stream of its own.
    TorchQNet(handle=h, device=d) wraps a model someone else owns (a learner's).  `reserve`: the largest n of any call.

    `layout` names the channel order the net sees, for every source: 'nchw_time' feeds the oldest frame as channel 0,
    'nhwc_slot' ring slot j as channel j (what the learner and DeepQLearningModel feed).  Use one throughout.

    A loss of one's own: net(states) - forward() - returns q [n, 3] with a grad_fn; loss.backward() runs
    the net's backward kernels on dloss/dq and leaves the raw gradients of all ten variables in the net's gradient buffer
    (grads()), step() clips and applies Adam.  One backward per step(): gradients are overwritten, not accumulated, and
    the states an env or a replay source was read from must stand until the backward (no env.step / reset, no
    replay.add in between).  Gradients with respect to the states do not exist."""

    def __init__(self, arch="f32", seed=2, device="cuda:0", env=None, reserve=MAX_STATES, handle=None):
        if arch not in _ARCHS:
            raise ValueError(f"arch must be 'f32' or 'bf16', not {arch!r}")
        if not 0 < reserve <= MAX_STATES:
            raise ValueError(f"reserve must be in 1..{MAX_STATES}")
        self.device = env.device if env is not None else _device(device)
        self.arch = arch
        if handle is None:
            self._m = qlx.DeepQLearningModel(seed, self.device.index, precision=_ARCHS[arch])
        else:
            self._m = qlx.DeepQLearningModel(handle=handle)
        self.h = self._m.h
        self._env = env   # with env=: the stream is the env's, keep it alive
        if env is not None:
            qlx._check(_L.qlx_model_share_stream(self.h, env.h))
            env._sharing.add(self)
        qlx._check(_L.qlx_model_reserve(self.h, reserve))
        self.reserved = reserve
        self._wrap_stream(_L.qlx_model_stream)
        self._anchor = torch.zeros((), dtype=torch.float32, device=self.device, requires_grad=True)
        self._pending = False   # a backward has filled the gradient buffer and no step() / discard_grad() followed
        self.reuse_activations = True   # False: every autograd backward runs the trunk forward again (ticket 0)
        self._grads = None
        self._head = None         # the attached qlx.WideHead (attach_head)
        self._head_grads = None
        self._dist_work = {}      # width -> the two work tensors of train_dist
        self._act_work = {}       # width -> the Z work tensor of act

    def close(self):
        head = getattr(self, "_head", None)
        if head is not None:   # before its model: a model with a live head cannot be destroyed
            head.close()
        self._head = self._head_grads = None
        m = getattr(self, "_m", None)
        if m is not None:
            m.close()
        self.h = None
        self._grads = None

    # ---- a wide output head beside the 512 -> 3 one ----

    def attach_head(self, width, seed=0):
        """Attach a dense layer 512 -> width (1..1024) on the trunk's a4 (qlx.WideHead; fp32 nets only, one per net) and
        return it.  forward(..., head=True) then returns (q, z), z float32 [n, width]; a loss of either or both
        backpropagates through one backward; step() steps the head's Wh and bh with the ten variables, each clipped by a
        norm of its own; head_grads() shows their gradients.  save_head / load_head are its persistence."""
        if self.h is None:
            raise QlError("the object is closed")
        self._head = qlx.WideHead(self._m, width, seed)
        self._head_grads = None
        return self._head

    @property
    def head(self):
        return self._head

    def _need_head(self):
        if self._head is None or self._head.h is None:
            raise RuntimeError("head=True needs an attached head: attach_head(width) first")
        return self._head

    def _forward_head(self, n, s, ins, env, replay, want_q=True):
        head = self._need_head()
        z = torch.empty((n, head.width), dtype=torch.float32, device=self.device)
        q = torch.empty((n, 3), dtype=torch.float32, device=self.device) if want_q else None
        self._run(env, replay, ins + (z, q),
                  lambda: _L.qlx_head_forward_dev(head.h, C.byref(s), n, z.data_ptr(), None if q is None else q.data_ptr()))
        return q, z

    def _forward_pass_head(self, obs, env, replay, indices, which, layout):
        s, n, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < n <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"n must be in 1..{min(MAX_BATCH, self.reserved)} for a differentiable forward")
        q, z = self._forward_head(n, s, ins, env, replay)
        return q, z, _Pass(s, n, ins, env, replay, self.forward_ticket())

    def backward_dz(self, dz, dq=None, ticket=0, obs=None, *, env=None, replay=None, indices=None, which="s",
                    layout="nchw_time", _pass=None):
        """qlx_head_backward_dev: the raw gradients of sum(dz * Z) + sum(dq * Q) into the two gradient buffers, dz float32
        [n, width], dq float32 [n, 3] or None (no Q term: dW4 and db4 come out zero).  `ticket` as in backward_dq."""
        head = self._need_head()
        if _pass is None:
            s, n, ins = self._source(obs, env, replay, indices, which, layout)
        else:
            s, n, ins, env, replay = _pass.src, _pass.n, _pass.ins, _pass.env, _pass.replay
        if not 0 < n <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"batch must be in 1..{min(MAX_BATCH, self.reserved)}")
        for name, t, shape in (("dz", dz, (n, head.width)), ("dq", dq, (n, 3))):
            if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != self.device):
                raise ValueError(f"{name} must be a tensor of shape {shape} on {self.device}")
        gz = dz.detach().to(torch.float32).contiguous()
        gq = None if dq is None else dq.detach().to(torch.float32).contiguous()
        self._run(env, replay, ins + (gz, gq),
                  lambda: _L.qlx_head_backward_dev(head.h, C.byref(s), gz.data_ptr(), None if gq is None else gq.data_ptr(),
                                                   n, ticket))
        self._pending = True

    def head_grads(self):
        """(dWh [512, width], dbh [width]) as float32 views of the head's gradient buffer; as grads()"""
        head = self._need_head()
        if self._head_grads is None:
            ptr, n = head.grads_dev()
            flat = torch.as_tensor(_DeviceFloats(ptr, n, head), device=self.device)
            k = qlx.HEAD_IN * head.width
            self._head_grads = (flat[:k].view(qlx.HEAD_IN, head.width), flat[k:])
        return self._head_grads

    # ---- distributional losses on the head: QR-DQN and C51 without a torch op on the update path ----

    def _dist(self, dist):
        head = self._need_head()
        if not isinstance(dist, _Dist):
            raise ValueError("dist must be a qlx_torch.Quantile or qlx_torch.Categorical")
        if dist.width != head.width:
            raise ValueError(f"3 * atoms = {dist.width} is not the head's width {head.width}")
        return head

    def _dist_batch(self, B, dist, actions, returns, discounts, terminals, z_next, a_star, weights):
        """(qlx.DistBatch, the tensors it points at) or ValueError before anything is launched"""
        ts = (_arg("actions", actions, self.device, torch.uint8, (B,)),
              _arg("returns", returns, self.device, torch.float32, (B,)),
              _arg("discounts", discounts, self.device, torch.float32, (B,)),
              _arg("terminals", terminals, self.device, torch.uint8, (B,)),
              _arg("z_next", z_next, self.device, torch.float32, (B, dist.width)),
              None if a_star is None else _arg("a_star", a_star, self.device, torch.uint8, (B,)),
              None if weights is None else _arg("weights", weights, self.device, torch.float32, (B,)))
        return qlx.DistBatch(*(None if t is None else t.data_ptr() for t in ts)), ts

    def head_values(self, z, dist, want=_WANT, out=None):
        """Q-values of head outputs z float32 [n, 3 * atoms] read as `dist` (Quantile or Categorical), in the shape of q():
        the tensors named in `want` - 'q' float32 [n, 3], 'actions' uint8 [n] (first argmax), 'max_q' float32 [n]."""
        head = self._dist(dist)
        if not isinstance(z, torch.Tensor) or z.dim() != 2:
            raise ValueError("z must be a 2-d tensor")
        n = z.shape[0]
        if not 0 < n <= self.reserved:
            raise ValueError(f"n must be in 1..{self.reserved} (the reserve)")
        zt = _arg("z", z.detach(), self.device, torch.float32, (n, dist.width))
        names = (want,) if isinstance(want, str) else tuple(want)
        out = dict(out or {})
        if not names or set(names) - set(_WANT) or set(out) - set(names):
            raise ValueError(f"want must name some of {_WANT}, and out only what want names")
        spec = dict(q=(torch.float32, (n, 3)), actions=(torch.uint8, (n,)), max_q=(torch.float32, (n,)))
        res = {k: (_arg(f"out[{k!r}]", out[k], self.device, *spec[k]) if k in out else
                   torch.empty(spec[k][1], dtype=spec[k][0], device=self.device)) for k in names}
        ptr = [res[k].data_ptr() if k in res else None for k in _WANT]
        self._run(None, None, (zt,) + tuple(res.values()),
                  lambda: _L.qlx_head_values_dev(head.h, C.byref(dist.c), zt.data_ptr(), n, *ptr))
        return res[want] if isinstance(want, str) else tuple(res[k] for k in names)

    def _dist_loss(self, z, dist, actions, returns, discounts, terminals, z_next, a_star, weights):
        head = self._dist(dist)
        if not isinstance(z, torch.Tensor) or z.dim() != 2:
            raise ValueError("z must be a 2-d tensor")
        B = z.shape[0]
        if not 0 < B <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"batch must be in 1..{min(MAX_BATCH, self.reserved)}")
        zt = _arg("z", z.detach(), self.device, torch.float32, (B, dist.width))
        batch, ts = self._dist_batch(B, dist, actions, returns, discounts, terminals, z_next, a_star, weights)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        dz = torch.empty((B, dist.width), dtype=torch.float32, device=self.device)
        sample_loss = torch.empty(B, dtype=torch.float32, device=self.device)
        a_out = torch.empty(B, dtype=torch.uint8, device=self.device)
        self._run(None, None, (zt,) + ts + (loss, dz, sample_loss, a_out),
                  lambda: _L.qlx_head_dist_loss_dev(head.h, C.byref(dist.c), zt.data_ptr(), C.byref(batch), B, dz.data_ptr(),
                                                    loss.data_ptr(), sample_loss.data_ptr(), a_out.data_ptr()))
        return loss, dz, sample_loss, a_out

    def dist_loss(self, z, dist, actions, returns, discounts, terminals, z_next, a_star=None, weights=None):
        """The distributional loss of head outputs z float32 [B, 3 * atoms] against the target net's z_next [B, 3 * atoms]:
        (loss, dz, sample_loss, a_star) - loss 0-d = mean of weights * sample_loss, dz = dloss/dz [B, 3 * atoms] (pass it to
        backward_dz), sample_loss float32 [B] (no weights: what update_priorities takes), a_star uint8 [B] (the one given,
        or the first argmax of the values of z_next).  actions, returns, discounts, terminals as TorchReplay.batch gives
        them.  When z carries a grad_fn (forward(head=True)), loss does too: loss.backward() hands dz * grad on to it."""
        args = (actions, returns, discounts, terminals, z_next, a_star, weights)
        if torch.is_grad_enabled() and isinstance(z, torch.Tensor) and z.requires_grad:
            return _DistLossFunction.apply(z, self, dist, args)
        return self._dist_loss(z, dist, *args)

    def train_dist(self, dist, actions, returns, discounts, terminals, z_next, a_star=None, weights=None, *, obs=None,
                   env=None, replay=None, indices=None, which="s", layout="nchw_time", want_sample_loss=False):
        """One whole update of the net and its head on B states in one call (qlx_head_dist_train_dev: the head's forward,
        the distributional loss, the backward, clip_by_norm and Adam): (loss, sample_loss), loss a 0-d float32 device
        tensor, sample_loss float32 [B] or None.  The two [B, 3 * atoms] work tensors are allocated once per net and width."""
        head = self._dist(dist)
        s, B, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < B <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"batch must be in 1..{min(MAX_BATCH, self.reserved)}")
        batch, ts = self._dist_batch(B, dist, actions, returns, discounts, terminals, z_next, a_star, weights)
        work = self._dist_work.get(dist.width)
        if work is None:
            rows = min(MAX_BATCH, self.reserved)
            work = self._dist_work[dist.width] = tuple(torch.empty((rows, dist.width), dtype=torch.float32, device=self.device)
                                                       for _ in range(2))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        sl = torch.empty(B, dtype=torch.float32, device=self.device) if want_sample_loss else None
        self._pending = False   # (the update overwrites the gradient buffers)
        self._run(env, replay, ins + ts + work + (loss, sl),
                  lambda: _L.qlx_head_dist_train_dev(head.h, C.byref(dist.c), C.byref(s), C.byref(batch), B, work[0].data_ptr(),
                                                     work[1].data_ptr(), loss.data_ptr(), None if sl is None else sl.data_ptr()))
        return loss, sl

    # ---- acting with, evaluating and checkpointing the head ----

    @staticmethod
    def _epsilon(epsilon):
        e = float(epsilon)
        if not (math.isfinite(e) and 0.0 <= e <= 1.0):
            raise ValueError("epsilon must be finite and in 0..1")
        return e

    def _select_outputs(self, n, want, out):
        """({name: tensor} with 'actions' always in it, the names asked for) or ValueError before anything is launched"""
        names = (want,) if isinstance(want, str) else tuple(want)
        out = dict(out or {})
        if not names or set(names) - set(_WANT) or set(out) - set(names):
            raise ValueError(f"want must name some of {_WANT}, and out only what want names")
        spec = dict(q=(torch.float32, (n, 3)), actions=(torch.uint8, (n,)), max_q=(torch.float32, (n,)))
        res = {k: (_arg(f"out[{k!r}]", out[k], self.device, *spec[k]) if k in out else
                   torch.empty(spec[k][1], dtype=spec[k][0], device=self.device)) for k in set(names) | {"actions"}}
        return res, names

    def select(self, z, dist, epsilon, seed, step, want="actions", out=None):
        """Epsilon-greedy actions of head outputs z float32 [n, 3 * atoms] read as `dist`, in one launch
        (qlx_head_select_dev): row r is random when epsilon > 0 and epsilon > a float64 draw of the stream (seed, r, step,
        qlx.P_ACT_DEV), then uniform over the three actions, else the first argmax of the values.  `want` and `out` as in
        head_values; 'max_q' and 'q' are the greedy values whatever was drawn.  With epsilon 0 this is head_values."""
        head = self._dist(dist)
        if not isinstance(z, torch.Tensor) or z.dim() != 2:
            raise ValueError("z must be a 2-d tensor")
        n = z.shape[0]
        if not 0 < n <= self.reserved:
            raise ValueError(f"n must be in 1..{self.reserved} (the reserve)")
        zt = _arg("z", z.detach(), self.device, torch.float32, (n, dist.width))
        eps = self._epsilon(epsilon)
        res, names = self._select_outputs(n, want, out)
        ptr = [res[k].data_ptr() if k in res else None for k in ("actions", "max_q", "q")]
        self._run(None, None, (zt,) + tuple(res.values()),
                  lambda: _L.qlx_head_select_dev(head.h, C.byref(dist.c), zt.data_ptr(), n, eps, seed, step, *ptr))
        return res[want] if isinstance(want, str) else tuple(res[k] for k in names)

    def act(self, dist, epsilon, seed, step, obs=None, *, env=None, replay=None, indices=None, which="s", layout="nchw_time",
            want="actions", out=None):
        """The acting step in one call (qlx_head_act_dev): the head's forward over the states, then select() on its output.
        The [reserve, 3 * atoms] work tensor that holds Z is allocated once per net and width."""
        head = self._dist(dist)
        s, n, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < n <= self.reserved:
            raise ValueError(f"n must be in 1..{self.reserved} (the reserve)")
        eps = self._epsilon(epsilon)
        res, names = self._select_outputs(n, want, out)
        work = self._act_work.get(dist.width)
        if work is None:
            work = self._act_work[dist.width] = torch.empty((self.reserved, dist.width), dtype=torch.float32, device=self.device)
        ptr = [res[k].data_ptr() if k in res else None for k in ("actions", "max_q", "q")]
        self._run(env, replay, ins + tuple(res.values()) + (work,),
                  lambda: _L.qlx_head_act_dev(head.h, C.byref(dist.c), C.byref(s), n, eps, seed, step, *ptr, work.data_ptr()))
        return res[want] if isinstance(want, str) else tuple(res[k] for k in names)

    def evaluate(self, evaluator, dist=None):
        """The summary of a qlx.Evaluator run of this net's policy: with `dist` the attached head's (Evaluator.run_head: the
        argmax of the head's values), without it the built-in 512 -> 3 head's (Evaluator.run).  The run is a host call on
        the net's stream: it waits for torch's current stream first and has finished when it returns."""
        if not isinstance(evaluator, qlx.Evaluator):
            raise ValueError("evaluator must be a qlx.Evaluator")
        if evaluator.h is None or self.h is None:
            raise QlError("the object is closed")
        head = None if dist is None else self._dist(dist)
        with self._ordered():
            return evaluator.run(self._m) if head is None else evaluator.run_head(head, dist.c)

    def save_head(self, path):
        """the attached head's weights, Adam slots and iterations into `path` (qlx_head_write_checkpoint); the ten model
        variables go through model.write_checkpoint"""
        head = self._need_head()
        with self._ordered():
            return head.write_checkpoint(path)

    def load_head(self, path):
        head = self._need_head()
        with self._ordered():
            head.read_checkpoint(path)

    @property
    def model(self):
        """the qlx.DeepQLearningModel underneath (host calls: get / set, checkpoints, iterations)"""
        return self._m

    def _source(self, obs, env, replay, indices, which, layout):
        """(StatesDev, n, the tensors it reads) or ValueError before anything is launched"""
        lay = _layout(layout)
        if which not in _WHICH:
            raise ValueError(f"which must be 's' or 's_next', not {which!r}")
        if (obs is not None) + (env is not None) + (replay is not None or indices is not None) != 1:
            raise ValueError("exactly one state source: obs, env or replay + indices")
        s = qlx.StatesDev(layout=lay, which=_WHICH[which])
        if obs is not None:
            if not isinstance(obs, torch.Tensor) or obs.dim() != 4:
                raise ValueError("obs must be a 4-d tensor")
            n = obs.shape[0]
            t = _arg("obs", obs, self.device, torch.uint8, (n,) + _STATE_SHAPE[lay])
            s.obs = t.data_ptr()
            return s, n, (t,)
        if env is not None:
            if env.device != self.device:
                raise ValueError(f"env must be on {self.device}")
            s.env = env.h
            return s, env.n, ()
        if replay is None or indices is None:
            raise ValueError("replay and indices go together")
        if replay.device != self.device:
            raise ValueError(f"replay must be on {self.device}")
        if not isinstance(indices, torch.Tensor) or indices.dim() != 1:
            raise ValueError("indices must be a 1-d tensor")
        n = indices.shape[0]
        t = _arg("indices", indices, self.device, torch.int64, (n,))
        s.replay, s.indices = replay.h, t.data_ptr()
        return s, n, (t,)

    def _others(self, env, replay):
        """the objects whose streams a call reads from: ordered like this one (a shared stream is entered once)"""
        seen, out = {self.stream.cuda_stream}, []
        for o in (env, replay):
            if o is not None and o.stream.cuda_stream not in seen:
                seen.add(o.stream.cuda_stream)
                out.append(o)
        return out

    def _run(self, env, replay, tensors, call):
        with contextlib.ExitStack() as stack:
            for o in self._others(env, replay):
                stack.enter_context(o._ordered())
            stack.enter_context(self._ordered(*tensors))
            qlx._check(call())

    def q(self, obs=None, *, env=None, replay=None, indices=None, which="s", layout="nchw_time", want=_WANT, out=None):
        """Q(s) of n states: the tensors named in `want`, in that order (one name: that tensor alone) - 'q' float32
        [n, 3], 'actions' uint8 [n] (first argmax), 'max_q' float32 [n].  `out`: a dict of tensors to write into, by those
        names.  A replay index >= len gives the Q of the all-zero state and an error at sync()."""
        s, n, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < n <= self.reserved:
            raise ValueError(f"n must be in 1..{self.reserved} (the reserve)")
        names = (want,) if isinstance(want, str) else tuple(want)
        out = dict(out or {})
        if not names or set(names) - set(_WANT) or set(out) - set(names):
            raise ValueError(f"want must name some of {_WANT}, and out only what want names")
        spec = dict(q=(torch.float32, (n, 3)), actions=(torch.uint8, (n,)), max_q=(torch.float32, (n,)))
        res = {k: (_arg(f"out[{k!r}]", out[k], self.device, *spec[k]) if k in out else
                   torch.empty(spec[k][1], dtype=spec[k][0], device=self.device)) for k in names}
        ptr = [res[k].data_ptr() if k in res else None for k in _WANT]
        self._run(env, replay, ins + tuple(res.values()), lambda: _L.qlx_model_q_dev(self.h, C.byref(s), n, *ptr))
        return res[want] if isinstance(want, str) else tuple(res[k] for k in names)

    def train(self, actions, y, weights=None, *, obs=None, env=None, replay=None, indices=None, which="s",
              layout="nchw_time", want_td_abs=False):
        """One update on B states with uint8 actions [B], float32 targets y [B] and optional float32 per-sample loss
        weights [B]: (loss, td_abs), loss a 0-d float32 device tensor, td_abs = |q_a - y| float32 [B] or None.  An action
        >= 3 trains as action 0 and gives an error at sync()."""
        s, B, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < B <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"batch must be in 1..{min(MAX_BATCH, self.reserved)}")
        a = _arg("actions", actions, self.device, torch.uint8, (B,))
        t = _arg("y", y, self.device, torch.float32, (B,))
        w = None if weights is None else _arg("weights", weights, self.device, torch.float32, (B,))
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        td = torch.empty(B, dtype=torch.float32, device=self.device) if want_td_abs else None
        self._pending = False   # (the update overwrites the gradient buffer)
        self._run(env, replay, ins + (a, t, w, loss, td),
                  lambda: _L.qlx_model_train_dev(self.h, C.byref(s), a.data_ptr(), t.data_ptr(), None if w is None else w.data_ptr(),
                                                 B, loss.data_ptr(), None if td is None else td.data_ptr()))
        return loss, td

    # ---- a loss written in torch: forward with a grad_fn, backward into the gradient buffer, step ----

    def forward(self, obs=None, *, env=None, replay=None, indices=None, which="s", layout="nchw_time", head=False):
        """q float32 [n, 3] (n <= 4096) of the states, differentiable: q carries a grad_fn whose backward runs the net's
        backward kernels.  Under torch.no_grad() this is q(want='q').  head=True (after attach_head): (q, z) with z float32
        [n, width] the wide head's output, from one trunk forward and with one backward for both; under torch.no_grad() the
        plain forward of up to `reserve` states."""
        if head:
            self._need_head()
            if not torch.is_grad_enabled():
                s, n, ins = self._source(obs, env, replay, indices, which, layout)
                if not 0 < n <= self.reserved:
                    raise ValueError(f"n must be in 1..{self.reserved} (the reserve)")
                return self._forward_head(n, s, ins, env, replay)
            return _QZFunction.apply(self._anchor, self, (obs, env, replay, indices, which, layout))
        if not torch.is_grad_enabled():
            return self.q(obs, env=env, replay=replay, indices=indices, which=which, layout=layout, want="q")
        return _QFunction.apply(self._anchor, self, (obs, env, replay, indices, which, layout))

    __call__ = forward

    def forward_ticket(self):
        """the ticket of the model's most recent forward pass (qlx_model_forward_ticket)"""
        t = C.c_uint64()
        qlx._check(_L.qlx_model_forward_ticket(self.h, C.byref(t)))
        return t.value

    def _forward_pass(self, obs, env, replay, indices, which, layout):
        s, n, ins = self._source(obs, env, replay, indices, which, layout)
        if not 0 < n <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"n must be in 1..{min(MAX_BATCH, self.reserved)} for a differentiable forward")
        q = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        self._run(env, replay, ins + (q,), lambda: _L.qlx_model_q_dev(self.h, C.byref(s), n, q.data_ptr(), None, None))
        return q, _Pass(s, n, ins, env, replay, self.forward_ticket())

    def _backward_pass(self, rec, grad_q, grad_z=None, head=False):
        if self.h is None:
            raise RuntimeError("backward through a closed TorchQNet")
        if self._pending:
            raise RuntimeError("a second backward before step() or discard_grad(): gradients are not accumulated")
        for o, count in rec.writes:
            if o.h is None or o.writes != count:
                raise RuntimeError(f"the {type(o).__name__} this forward read was stepped, reset, pushed to or closed before "
                                   "the backward: its states are read in place")
        ticket = rec.ticket if self.reuse_activations else 0
        if head:
            if grad_z is None:
                grad_z = torch.zeros((rec.n, self._need_head().width), dtype=torch.float32, device=self.device)
            self.backward_dz(grad_z, grad_q, ticket, _pass=rec)
        else:
            self.backward_dq(grad_q, ticket, _pass=rec)

    def backward_dq(self, dq, ticket=0, obs=None, *, env=None, replay=None, indices=None, which="s", layout="nchw_time",
                    _pass=None):
        """qlx_model_backward_dev: the raw gradients of sum(dq * Q(states)) into the gradient buffer, dq float32 [n, 3].
        `ticket`: that of the forward over these very states (forward_ticket() right after it) to reuse its activations;
        0 runs the trunk forward again.  The autograd path calls this; on its own it makes none of that path's checks."""
        if _pass is None:
            s, n, ins = self._source(obs, env, replay, indices, which, layout)
        else:
            s, n, ins, env, replay = _pass.src, _pass.n, _pass.ins, _pass.env, _pass.replay
        if not 0 < n <= min(MAX_BATCH, self.reserved):
            raise ValueError(f"batch must be in 1..{min(MAX_BATCH, self.reserved)}")
        if not isinstance(dq, torch.Tensor) or tuple(dq.shape) != (n, 3) or dq.device != self.device:
            raise ValueError(f"dq must be a tensor of shape {(n, 3)} on {self.device}")
        g = dq.detach().to(torch.float32).contiguous()
        self._run(env, replay, ins + (g,), lambda: _L.qlx_model_backward_dev(self.h, C.byref(s), g.data_ptr(), n, ticket))
        self._pending = True

    def step(self, grads_written=False):
        """clip_by_norm per variable + Adam on the gradient buffer, iterations + 1.  grads_written: the buffer was modified
        through grads() since the backward (its clip norms are then taken from the buffer as it stands).  After a backward
        through an attached head (forward(head=True), backward_dz) the head's Wh and bh are stepped as well."""
        with self._ordered():
            qlx._check(_L.qlx_model_step_dev(self.h, qlx.STEP_GRADS_WRITTEN if grads_written else 0))
        self._pending = False

    def discard_grad(self):
        """drop the pending gradient, so that another backward may run without a step()"""
        self._pending = False

    def grads(self):
        """the ten variables' gradients as float32 views of the gradient buffer, in the Keras shapes (qlx.VAR_SHAPES).
        They show what the model's stream has written: read or write them between a backward and step(), and pass
        step(grads_written=True) after a write.  Valid until close()."""
        if self.h is None:
            raise QlError("the object is closed")
        if self._grads is None:
            p, n = C.c_void_p(), C.c_uint64()
            qlx._check(_L.qlx_model_grads_dev(self.h, C.byref(p), C.byref(n)))
            flat = torch.as_tensor(_DeviceFloats(p.value, n.value, self._m), device=self.device)
            views, off = [], 0
            for shape in qlx.VAR_SHAPES:
                k = 1
                for d in shape:
                    k *= d
                views.append(flat[off:off + k].view(shape))
                off += k
            assert off == n.value
            self._grads = tuple(views)
        return self._grads

    def copy_weights_from(self, other):
        """the weights of `other` (a TorchQNet), as a target-network sync: no host synchronisation"""
        if not isinstance(other, TorchQNet) or other.device != self.device:
            raise ValueError(f"other must be a TorchQNet on {self.device}")
        if other.h is None:
            raise QlError("the object is closed")
        mine, theirs = self._head, other._head
        if mine is not None and theirs is not None and mine.width != theirs.width:
            raise ValueError(f"the heads have different widths ({mine.width} and {theirs.width})")
        with self._ordered():
            qlx._check(_L.qlx_model_copy_weights_dev(self.h, other.h))
            if mine is not None and theirs is not None:   # both nets have a head: it is part of the sync
                qlx._check(_L.qlx_head_copy_weights_dev(mine.h, theirs.h))

    def sync(self):
        """wait for the model's stream; QlError, once, if a call since the last sync met an index >= len or an action >= 3"""
        qlx._check(_L.qlx_model_sync(self.h))
