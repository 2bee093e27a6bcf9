"""Fused policy inference: the reference's Agent
(scripts/agent.py:108-154, 32 channels, 2 layers, buckets [2,8,3,2,2,2]) run
by one gfx950 kernel (bb_policy_forward, csrc/bb_policy.hip; at the 184 / 264 /
344 / 424-float rows of 4, 6, 8 and 10 agents bb_policy_forward_wide,
csrc/bb_policy_wide.hip) that writes its actions straight into the simulator's
action tensor -- the `actions, log_probs, values = agent(obs)` +
`actions[:, i] = a` pair of scripts/ppo.py:67 / scripts/env.py:147 without a
round trip through torch.  The wide networks also have the minibatch loss and
gradient in one call (FusedPolicy.ppo_grad_wide, bb_policy_ppo_grad_wide,
csrc/bb_policy_grad_wide.hip), the clip + Adam step behind it
(optimizer_step / ppo_minibatch / ppo_update, csrc/bb_policy_step_wide.hip) and
the advantage phase (compute_advantages, csrc/bb_advantages_wide.hip); only
the fused rollout is 128-wide only.

FusedPolicy.from_agent(agent) snapshots the weights of any torch module with
the reference Agent's layout (obs_norm.mean/var, backbone Linear/LayerNorm,
actor, critic).  The packed weights follow the agent through
optimizer_step / ppo_minibatch / ppo_update (clipping, Adam and the repack in
one launch); after a torch optimizer step, or after compute_advantages (new
observation statistics), call refresh().
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .madrona import ExecMode

BUCKETS = (2, 8, 3, 2, 2, 2)
IN, HID, LOGITS, HEAD = 128, 32, 19, 32
WIDTHS = (128, 184, 264, 344, 424)  # bb_obs_width(N), N = 2, 4, 6, 8, 10: the first layer's input widths served
PARAMS = HID * IN + HID * HID + 6 * HID + (LOGITS + 1) * (HID + 1)  # 5 972


class _ObsNorm(torch.nn.Module):
    """RunningMeanStd's state (scripts/agent.py:19-26): float64 mean / var, eps."""

    def __init__(self, dim: int):
        super().__init__()
        self.epsilon = 1e-5
        self.register_buffer("mean", torch.zeros(dim, dtype=torch.float64))
        self.register_buffer("var", torch.ones(dim, dtype=torch.float64))


class RunningStats:
    """RunningMeanStd's three buffers (scripts/agent.py:24-26) at their initial
    values -- float64 mean 0 [dim], var 1 [dim], count 1 [] -- for
    FusedPolicy.compute_advantages to update in place."""

    def __init__(self, dim: int, device=None):
        self.mean = torch.zeros(dim, dtype=torch.float64, device=device)
        self.var = torch.ones(dim, dtype=torch.float64, device=device)
        self.count = torch.ones((), dtype=torch.float64, device=device)


def make_agent(seed: int = 0, input_dim: int = IN) -> torch.nn.Module:
    """A torch module with the reference Agent's layout and initialisation
    (scripts/agent.py:97-131: Kaiming-normal backbone, orthogonal heads at gain
    0.01, zero biases, identity observation normaliser) -- random weights of
    that architecture for benchmarks and tests (no checkpoints here).  input_dim:
    the observation width, envs.get_input_dim() (128 for the 2-agent game)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.nn.Module()
    m.action_buckets = list(BUCKETS)
    m.backbone = torch.nn.Sequential(torch.nn.Linear(input_dim, HID), torch.nn.LayerNorm(HID), torch.nn.ReLU(),
                                     torch.nn.Linear(HID, HID), torch.nn.LayerNorm(HID), torch.nn.ReLU())
    m.actor = torch.nn.Linear(HID, LOGITS)
    m.critic = torch.nn.Linear(HID, 1)
    m.obs_norm = _ObsNorm(input_dim)
    with torch.no_grad():
        for lin in (m.backbone[0], m.backbone[3]):
            torch.nn.init.kaiming_normal_(lin.weight, torch.nn.init.calculate_gain("relu"), generator=g)
            lin.bias.zero_()
        for lin in (m.actor, m.critic):
            torch.nn.init.orthogonal_(lin.weight, gain=0.01, generator=g)
            lin.bias.zero_()
    return m


def agent_from_state_dict(state_dict: dict, device=None) -> torch.nn.Module:
    """A module of the reference Agent's layout holding `state_dict` -- the
    keys Agent.state_dict() / a checkpoint written by scripts/ppo.py has
    (backbone.{0,1,3,4}.*, actor.*, critic.*, obs_norm.mean/var; the
    value_norm / count buffers are not used by inference).  Load checkpoints
    with torch.load(path, weights_only=True), as Agent.load does
    (scripts/agent.py:180-182)."""
    if "backbone.0.weight" not in state_dict:
        raise KeyError("state_dict lacks ['backbone.0.weight']")
    m = make_agent(0, int(torch.as_tensor(state_dict["backbone.0.weight"]).shape[-1]))  # the width it was trained at
    own = m.state_dict()
    missing = [k for k in own if k not in state_dict]
    if missing:
        raise KeyError(f"state_dict lacks {missing}")
    with torch.no_grad():
        for k, v in own.items():
            src = torch.as_tensor(state_dict[k])
            if tuple(src.shape) != tuple(v.shape):
                raise ValueError(f"{k}: shape {tuple(src.shape)}, expected {tuple(v.shape)}")
            v.copy_(src.to(v.dtype))
    return m if device is None else m.to(device)


class AdamState:
    """torch.optim.Adam's state for the agent's 5 972 parameter elements, zeroed,
    for FusedPolicy.optimizer_step / ppo_minibatch / ppo_update: exp_avg and
    exp_avg_sq float32 [5972] in the gradient's packed order (w1 b1 ln1_w ln1_b
    w2 b2 ln2_w ln2_b actor.w critic.w actor.b critic.b), step int64 [1], and
    the kernels' ticket int32 [1] (0 between calls).  in_dim: the policy's
    input width; a wider first layer has 32 (in_dim - 128) more elements (w1
    first, every later offset that much further on)."""

    def __init__(self, device=None, *, in_dim: int = IN):
        n = PARAMS + HID * (int(in_dim) - IN)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=device)
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=device)


class FusedPolicy:
    def __init__(self, device: torch.device):
        self.device = torch.device(device)
        self._tensors = {}

    @classmethod
    def from_agent(cls, agent, device=None) -> "FusedPolicy":
        dev = device or next(agent.parameters()).device
        p = cls(dev)
        p.agent = agent
        p.refresh()
        return p

    @torch.no_grad()
    def refresh(self) -> None:
        """Re-read the agent's weights (after an update)."""
        a = self.agent
        lin = [m for m in a.backbone if isinstance(m, torch.nn.Linear)]
        lns = [m for m in a.backbone if isinstance(m, torch.nn.LayerNorm)]
        if (len(lin) != 2 or lin[0].in_features not in WIDTHS or lin[0].out_features != HID
                or lin[1].out_features != HID or a.actor.out_features != LOGITS
                or tuple(a.action_buckets) != BUCKETS or tuple(a.obs_norm.mean.shape) != (lin[0].in_features,)):
            raise ValueError("FusedPolicy supports the reference configuration: input 128 (or the 184, 264, 344, 424 "
                             "of 4 to 10 agents), num_channels 32, num_layers 2, buckets [2, 8, 3, 2, 2, 2] "
                             "(scripts/env.py:107)")
        self.in_dim = lin[0].in_features
        dev, f32 = self.device, torch.float32

        def t(x):
            return x.detach().to(device=dev, dtype=f32).contiguous()
        # RunningMeanStd.forward (agent.py:29-35): mean/var cast to f32, var + eps, rsqrt
        mean = a.obs_norm.mean.to(f32)
        var = a.obs_norm.var.to(f32) + a.obs_norm.epsilon
        head_w = torch.zeros((HEAD, HID), dtype=f32, device=dev)
        head_b = torch.zeros((HEAD,), dtype=f32, device=dev)
        head_w[:LOGITS] = t(a.actor.weight)
        head_w[LOGITS] = t(a.critic.weight)[0]
        head_b[:LOGITS] = t(a.actor.bias)
        head_b[LOGITS] = t(a.critic.bias)[0]
        self._tensors = {
            "obs_mean": t(mean), "obs_inv": t(torch.rsqrt(var.to(dev))),
            "w1": t(lin[0].weight), "b1": t(lin[0].bias), "ln1_w": t(lns[0].weight), "ln1_b": t(lns[0].bias),
            "w2": t(lin[1].weight), "b2": t(lin[1].bias), "ln2_w": t(lns[1].weight), "ln2_b": t(lns[1].bias),
            "head_w": head_w, "head_b": head_b,
        }
        self._w = _lib.PolicyWeights(**{k: v.data_ptr() for k, v in self._tensors.items()})

    def to(self, device) -> "FusedPolicy":
        """A copy of the packed weights on another device (same bits)."""
        p = FusedPolicy(device)
        p.agent = getattr(self, "agent", None)
        p.in_dim = self.in_dim
        p._tensors = {k: v.to(p.device).contiguous() for k, v in self._tensors.items()}
        p._w = _lib.PolicyWeights(**{k: v.data_ptr() for k, v in p._tensors.items()})
        return p

    def _stream(self):
        if self.device.type == "cuda":
            return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return ctypes.c_void_p(None)

    def forward_into(self, obs: torch.Tensor, actions: torch.Tensor, log_prob: torch.Tensor = None,
                     value: torch.Tensor = None, stochastic: bool = True, seed: int = 0, step: int = 0) -> None:
        """obs [R, >= in_dim] float32 rows (any row stride, e.g. obs_tensor[:, agent])
        of the simulator the agent was built for: the first in_dim floats of a row
        are the network's input, so in_dim must be that simulator's observation
        width, bb_obs_width(N) (128, 184, 264, 344, 424 for 2 to 10 agents; act_all
        checks it); actions [R, 6] int32 rows (any row stride, e.g.
        action_tensor[:, agent])."""
        rows, in_dim = obs.shape[0], self.in_dim
        if obs.dim() != 2 or obs.shape[1] < in_dim or obs.stride(1) != 1 or obs.dtype != torch.float32:
            raise ValueError(f"obs must be float32 [rows, >={in_dim}] with unit column stride")
        if (actions.dim() != 2 or actions.shape != (rows, 6) or actions.stride(1) != 1
                or actions.dtype != torch.int32):
            raise ValueError("actions must be int32 [rows, 6] with unit column stride")
        for t in (obs, actions, log_prob, value):
            if t is not None and t.device != self.device:
                raise ValueError("all tensors must live on the policy's device")
        for t in (log_prob, value):
            if t is not None and (t.shape != (rows,) or not t.is_contiguous() or t.dtype != torch.float32):
                raise ValueError("log_prob / value must be contiguous float32 [rows]")
        mode = ExecMode.CUDA if self.device.type == "cuda" else ExecMode.CPU
        lib = _lib.load()
        # 128: bb_policy_forward, as ever; the wider rows: bb_policy_forward_wide
        entry = lib.bb_policy_forward if in_dim == IN else lib.bb_policy_forward_wide
        width = () if in_dim == IN else (in_dim,)
        _lib.check(entry(
            ctypes.byref(self._w), *width, int(mode), self.device.index if self.device.index is not None else -1,
            ctypes.c_void_p(obs.data_ptr()), rows, obs.stride(0), ctypes.c_void_p(actions.data_ptr()),
            actions.stride(0), ctypes.c_void_p(None if log_prob is None else log_prob.data_ptr()),
            ctypes.c_void_p(None if value is None else value.data_ptr()), 1 if stochastic else 0,
            int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, self._stream()), "policy_forward")

    def __call__(self, obs: torch.Tensor, stochastic: bool = True, seed: int = 0, step: int = 0):
        """Agent.forward's outputs (actions int32 [R, 6], log_probs [R], values [R])."""
        rows = obs.shape[0]
        actions = torch.empty((rows, 6), dtype=torch.int32, device=self.device)
        lp = torch.empty((rows,), dtype=torch.float32, device=self.device)
        v = torch.empty((rows,), dtype=torch.float32, device=self.device)
        self.forward_into(obs, actions, lp, v, stochastic, seed, step)
        return actions, lp, v

    def act(self, sim, agent_idx: int, log_prob: torch.Tensor = None, value: torch.Tensor = None,
            stochastic: bool = True, seed: int = 0, step: int = 0) -> None:
        """Observe agent `agent_idx` of every world and write its actions into the
        simulator's action tensor (env.py:147's `actions[:, i] = a`), on the device."""
        obs = sim.observations_tensor().to_torch()[:, agent_idx]
        act = sim.action_tensor().to_torch()[:, agent_idx]
        self.forward_into(obs, act, log_prob, value, stochastic, seed, step)

    def act_all(self, sim, log_prob: torch.Tensor = None, value: torch.Tensor = None, stochastic: bool = True,
                seed: int = 0, step: int = 0) -> None:
        """One shared policy for every agent of every world, in one launch: the
        [W * N, obs_width] view of the observation tensor into the [W * N, 6] view
        of the action tensor (row w * N + i: agent i of world w; log_prob / value
        [W * N]).  The policy's in_dim must be the simulator's observation width."""
        obs = sim.observations_tensor().to_torch()
        if obs.shape[-1] != self.in_dim:
            raise ValueError(f"a {self.in_dim}-input policy cannot act for a simulator of {obs.shape[1]} agents "
                             f"(observation width {obs.shape[-1]})")
        act = sim.action_tensor().to_torch()
        self.forward_into(obs.view(-1, obs.shape[-1]), act.view(-1, 6), log_prob, value, stochastic, seed, step)

    def _require_128(self, what: str) -> None:
        if self.in_dim != IN:
            raise ValueError(f"{what} is built for the 128-wide configuration (the 2-agent game); this policy has "
                             f"{self.in_dim} inputs (ppo_grad_wide, optimizer_step, ppo_minibatch, ppo_update and "
                             "compute_advantages serve it)")

    # ------------------------------------------------------------- PPO update
    def ppo_grad(self, obs: torch.Tensor, actions: torch.Tensor, log_prob: torch.Tensor, value: torch.Tensor,
                 advantages: torch.Tensor, returns: torch.Tensor, idx: torch.Tensor = None, clip_coef: float = 0.2,
                 vf_coef: float = 1.0, ent_coef: float = 0.01) -> torch.Tensor:
        """One minibatch of update_policy up to loss.backward() (scripts/ppo.py:190-213,
        clip_vloss) in one pass on the device, bb_policy_ppo_grad: the rows `idx`
        (int64 [M], mb_inds; None: all R) of the rollout buffer's flat views -- obs
        float32 [R, 128], actions int32 [R, 6], log_prob / value / advantages /
        returns float32 [R] (scripts/buffers.py:25-33; the rollout_buffers tensors
        reshape to them without a copy) -- are gathered by the kernel, and the
        gradient of ppo.py:210's loss at the weights last packed by refresh() is
        left in .grad of the agent's 12 parameter tensors (overwritten), for
        clip_grad_norm_ and optimizer.step() to go on from.  Returns a float32 [4]
        tensor on the device: loss, pg_loss, c_loss before vf_coef, mean entropy
        (no host synchronisation).  head_grad keeps the packed head's gradient
        ([32, 32] and [32]: rows 0-18 the actor, 19 the critic, 20-31 zero)."""
        self._require_128("ppo_grad")
        batch, m = self._ppo_args(obs, actions, log_prob, value, advantages, returns, idx)
        direct = self._params(True)[:8]
        dev, f32, a = self.device, torch.float32, self.agent
        lib = _lib.load()
        cuda = dev.type == "cuda"
        need = lib.bb_policy_ppo_grad_workspace_bytes(m) if cuda else 0
        if getattr(self, "_ppo_ws", None) is None or self._ppo_ws.numel() * 4 < need:
            self._ppo_ws = torch.empty((max(need, 4) // 4,), dtype=f32, device=dev)
        if getattr(self, "head_grad", None) is None:
            self.head_grad = (torch.zeros((HEAD, HID), dtype=f32, device=dev), torch.zeros((HEAD,), dtype=f32, device=dev))
        hw, hb = self.head_grad
        loss4 = torch.empty((4,), dtype=f32, device=dev)
        coef = _lib.PpoCoef(float(clip_coef), float(vf_coef), float(ent_coef))
        grads = _lib.PolicyGrads(*[p.grad.data_ptr() for p in direct], hw.data_ptr(), hb.data_ptr())
        _lib.check(lib.bb_policy_ppo_grad(
            ctypes.byref(self._w), int(ExecMode.CUDA if cuda else ExecMode.CPU),
            dev.index if dev.index is not None else -1, ctypes.byref(batch), ctypes.byref(coef), ctypes.byref(grads),
            ctypes.c_void_p(loss4.data_ptr()), ctypes.c_void_p(self._ppo_ws.data_ptr() if cuda else None),
            need, self._stream()), "policy_ppo_grad")
        a.actor.weight.grad.copy_(hw[:LOGITS])
        a.critic.weight.grad.copy_(hw[LOGITS:LOGITS + 1])
        a.actor.bias.grad.copy_(hb[:LOGITS])
        a.critic.bias.grad.copy_(hb[LOGITS:LOGITS + 1])
        return loss4

    def ppo_grad_wide(self, obs: torch.Tensor, actions: torch.Tensor, log_prob: torch.Tensor, value: torch.Tensor,
                      advantages: torch.Tensor, returns: torch.Tensor, idx: torch.Tensor = None,
                      clip_coef: float = 0.2, vf_coef: float = 1.0, ent_coef: float = 0.01) -> torch.Tensor:
        """ppo_grad for a policy of 184, 264, 344 or 424 inputs (the 2v2 to 5v5
        games), bb_policy_ppo_grad_wide: the same contract with obs float32
        [R, in_dim] -- the rows `idx` gathered by the kernels, the gradient left in
        .grad of the agent's 12 parameters (backbone[0].weight.grad is [32, in_dim]),
        head_grad kept, float32 [4] returned on the device, no host
        synchronisation.  optimizer_step(state) takes the step from these
        gradients; ppo_minibatch / ppo_update run both without the reduce in
        between (only rollout remains 128-wide)."""
        if self.in_dim == IN:
            raise ValueError("ppo_grad_wide serves the 184, 264, 344 and 424-input policies; this one has 128 inputs: "
                             "use ppo_grad")
        width = self.in_dim
        batch, m = self._ppo_args(obs, actions, log_prob, value, advantages, returns, idx, width)
        direct = self._params(True, width)[:8]
        dev, f32, a = self.device, torch.float32, self.agent
        lib = _lib.load()
        cuda = dev.type == "cuda"
        need = lib.bb_policy_ppo_grad_wide_workspace_bytes(width, m) if cuda else 0
        if getattr(self, "_ppo_ws", None) is None or self._ppo_ws.numel() * 4 < need:
            self._ppo_ws = torch.empty((max(need, 4) // 4,), dtype=f32, device=dev)
        if getattr(self, "head_grad", None) is None:
            self.head_grad = (torch.zeros((HEAD, HID), dtype=f32, device=dev), torch.zeros((HEAD,), dtype=f32, device=dev))
        hw, hb = self.head_grad
        loss4 = torch.empty((4,), dtype=f32, device=dev)
        coef = _lib.PpoCoef(float(clip_coef), float(vf_coef), float(ent_coef))
        grads = _lib.PolicyGrads(*[p.grad.data_ptr() for p in direct], hw.data_ptr(), hb.data_ptr())
        _lib.check(lib.bb_policy_ppo_grad_wide(
            ctypes.byref(self._w), width, int(ExecMode.CUDA if cuda else ExecMode.CPU),
            dev.index if dev.index is not None else -1, ctypes.byref(batch), ctypes.byref(coef), ctypes.byref(grads),
            ctypes.c_void_p(loss4.data_ptr()), ctypes.c_void_p(self._ppo_ws.data_ptr() if cuda else None),
            need, self._stream()), "policy_ppo_grad_wide")
        a.actor.weight.grad.copy_(hw[:LOGITS])
        a.critic.weight.grad.copy_(hw[LOGITS:LOGITS + 1])
        a.actor.bias.grad.copy_(hb[:LOGITS])
        a.critic.bias.grad.copy_(hb[LOGITS:LOGITS + 1])
        return loss4

    def _ppo_args(self, obs, actions, log_prob, value, advantages, returns, idx, width: int = IN):
        """ppo_grad's checks of the batch (obs rows of `width` floats): its descriptor and M."""
        dev, f32 = self.device, torch.float32
        if obs.dim() != 2 or obs.shape[1] != width or obs.dtype != f32 or not obs.is_contiguous():
            raise ValueError(f"obs must be a contiguous float32 [rows, {width}] tensor")
        rows = obs.shape[0]
        if tuple(actions.shape) != (rows, 6) or actions.dtype != torch.int32 or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous int32 [rows, 6] tensor")
        for t in (log_prob, value, advantages, returns):
            if tuple(t.shape) != (rows,) or t.dtype != f32 or not t.is_contiguous():
                raise ValueError("log_prob, value, advantages and returns must be contiguous float32 [rows]")
        if idx is not None and (idx.dim() != 1 or idx.dtype != torch.int64 or not idx.is_contiguous()):
            raise ValueError("idx must be a contiguous int64 [M] tensor")
        m = rows if idx is None else idx.shape[0]
        if rows < 1 or m < 1:
            raise ValueError("an empty minibatch")
        for t in (obs, actions, log_prob, value, advantages, returns, idx):
            if t is not None and t.device != dev:
                raise ValueError("all tensors must live on the policy's device")
        batch = _lib.PpoBatch(obs.data_ptr(), actions.data_ptr(), log_prob.data_ptr(), value.data_ptr(),
                              advantages.data_ptr(), returns.data_ptr(), None if idx is None else idx.data_ptr(),
                              rows, m)
        return batch, m

    def _params(self, make_grads: bool, width: int = IN) -> list:
        """The agent's 12 parameters in agent.parameters() order (w1 [32, width] b1
        ln1_w ln1_b w2 b2 ln2_w ln2_b actor.w actor.b critic.w critic.b), float32 on
        the policy's device, each with a contiguous .grad (made if make_grads)."""
        a, dev = self.agent, self.device
        lin = [mod for mod in a.backbone if isinstance(mod, torch.nn.Linear)]
        lns = [mod for mod in a.backbone if isinstance(mod, torch.nn.LayerNorm)]
        ps = [lin[0].weight, lin[0].bias, lns[0].weight, lns[0].bias, lin[1].weight, lin[1].bias, lns[1].weight,
              lns[1].bias, a.actor.weight, a.actor.bias, a.critic.weight, a.critic.bias]
        if tuple(ps[0].shape) != (HID, width) or tuple(ps[4].shape) != (HID, HID) or a.actor.out_features != LOGITS:
            raise ValueError(f"FusedPolicy supports the reference configuration: input {width}, num_channels 32, "
                             "num_layers 2, buckets [2, 8, 3, 2, 2, 2] (scripts/env.py:107)")
        for p in ps:
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError("the agent's parameters must be float32 on the policy's device")
            if make_grads and (p.grad is None or not p.grad.is_contiguous()):
                p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if p.grad is None or not p.grad.is_contiguous():
                raise ValueError("every parameter needs a contiguous .grad (run a backward first)")
        return ps

    def _step_args(self, state: "AdamState", lr, max_grad_norm, betas, eps, make_grads: bool):
        if not isinstance(state, AdamState) or state.exp_avg.device != self.device:
            raise ValueError("state must be an AdamState on the policy's device")
        n = PARAMS + HID * (self.in_dim - IN)
        if state.exp_avg.numel() != n or state.exp_avg_sq.numel() != n:
            raise ValueError(f"a {self.in_dim}-input policy needs AdamState(device, in_dim={self.in_dim}): {n} "
                             "elements")
        ps = self._params(make_grads, self.in_dim)
        if any(not p.is_contiguous() for p in ps):
            raise ValueError("the agent's parameters must be contiguous")
        return (_lib.PolicyParams(*[p.data_ptr() for p in ps]), _lib.PolicyParams(*[p.grad.data_ptr() for p in ps]),
                _lib.AdamStatePtrs(state.exp_avg.data_ptr(), state.exp_avg_sq.data_ptr(), state.step.data_ptr(),
                                   state.ticket.data_ptr()),
                _lib.AdamHyper(float(lr), float(betas[0]), float(betas[1]), float(eps), float(max_grad_norm)))

    @torch.no_grad()
    def optimizer_step(self, state: "AdamState", lr: float = 3e-4, max_grad_norm: float = 1.0,
                       betas=(0.9, 0.999), eps: float = 1e-8) -> torch.Tensor:
        """clip_grad_norm_(agent.parameters(), max_grad_norm) + Adam.step() +
        refresh() (scripts/ppo.py:214-215) after any backward, in one launch,
        bb_policy_adam_step: the 12 .grad tensors are left clipped, `state` and the
        parameters take torch.optim.Adam's step (defaults: no weight decay, no
        amsgrad), and the new parameters are stored into the packed weights too
        (the observation statistics are not: refresh() after compute_advantages
        as before).  Returns float32 [2] on the device: the gradient norm before
        clipping and the clip factor (no host synchronisation).  At 184 to 424
        inputs bb_policy_adam_step_wide, with AdamState(device, in_dim=...)."""
        params, grads, st, hyper = self._step_args(state, lr, max_grad_norm, betas, eps, False)
        dev, lib = self.device, _lib.load()
        out2 = torch.empty((2,), dtype=torch.float32, device=dev)
        wide = self.in_dim != IN
        entry, width = (lib.bb_policy_adam_step_wide, (self.in_dim,)) if wide else (lib.bb_policy_adam_step, ())
        _lib.check(entry(
            ctypes.byref(self._w), *width, int(ExecMode.CUDA if dev.type == "cuda" else ExecMode.CPU),
            dev.index if dev.index is not None else -1, ctypes.byref(params), ctypes.byref(grads), ctypes.byref(st),
            ctypes.byref(hyper), ctypes.c_void_p(out2.data_ptr()), self._stream()), "policy_adam_step")
        return out2

    @torch.no_grad()
    def ppo_minibatch(self, obs: torch.Tensor, actions: torch.Tensor, log_prob: torch.Tensor, value: torch.Tensor,
                      advantages: torch.Tensor, returns: torch.Tensor, idx: torch.Tensor, state: "AdamState",
                      clip_coef: float = 0.2, vf_coef: float = 1.0, ent_coef: float = 0.01, lr: float = 3e-4,
                      max_grad_norm: float = 1.0, betas=(0.9, 0.999), eps: float = 1e-8) -> torch.Tensor:
        """One whole minibatch of update_policy (scripts/ppo.py:190-215): ppo_grad's
        pass (same arguments and checks), then optimizer_step's, as two launches
        (bb_policy_ppo_step) with no torch op between them -- the bits of
        ppo_grad() followed by optimizer_step().  Returns float32 [6] on the
        device: loss, pg_loss, c_loss, entropy, gradient norm before clipping,
        clip factor.  At 184 to 424 inputs bb_policy_ppo_step_wide: the bits of
        ppo_grad_wide() followed by optimizer_step()."""
        wide = self.in_dim != IN
        batch, m = self._ppo_args(obs, actions, log_prob, value, advantages, returns, idx, self.in_dim)
        params, grads, st, hyper = self._step_args(state, lr, max_grad_norm, betas, eps, True)
        dev, lib = self.device, _lib.load()
        cuda = dev.type == "cuda"
        entry, width = (lib.bb_policy_ppo_step_wide, (self.in_dim,)) if wide else (lib.bb_policy_ppo_step, ())
        query = lib.bb_policy_ppo_step_wide_workspace_bytes if wide else lib.bb_policy_ppo_step_workspace_bytes
        need = query(*width, m) if cuda else 0
        if getattr(self, "_ppo_ws", None) is None or self._ppo_ws.numel() * 4 < need:
            self._ppo_ws = torch.empty((max(need, 4) // 4,), dtype=torch.float32, device=dev)
        out6 = torch.empty((6,), dtype=torch.float32, device=dev)
        coef = _lib.PpoCoef(float(clip_coef), float(vf_coef), float(ent_coef))
        _lib.check(entry(
            ctypes.byref(self._w), *width, int(ExecMode.CUDA if cuda else ExecMode.CPU),
            dev.index if dev.index is not None else -1, ctypes.byref(batch), ctypes.byref(coef), ctypes.byref(params),
            ctypes.byref(grads), ctypes.byref(st), ctypes.byref(hyper), ctypes.c_void_p(out6.data_ptr()),
            ctypes.c_void_p(self._ppo_ws.data_ptr() if cuda else None), need, self._stream()), "policy_ppo_step")
        return out6

    def ppo_update(self, obs: torch.Tensor, actions: torch.Tensor, log_prob: torch.Tensor, value: torch.Tensor,
                   advantages: torch.Tensor, returns: torch.Tensor, state: "AdamState", update_epochs: int = 4,
                   num_minibatches: int = 4, perms: torch.Tensor = None, **kw) -> torch.Tensor:
        """update_policy (scripts/ppo.py:180-216) over the flat buffer views of
        ppo_grad: per epoch a permutation of the R rows (row e of `perms`, int64
        [update_epochs, R], or torch.randperm on the device), minibatches of
        R // num_minibatches rows at range(0, R, minibatch_size) -- a short last
        one when R is not divisible, as ppo.py:188 has it -- each one
        ppo_minibatch(**kw).  Returns float32 [steps, 6], one row per minibatch."""
        rows = obs.shape[0]
        mb = rows // int(num_minibatches)
        if mb < 1:
            raise ValueError("fewer rows than minibatches")
        if perms is not None and (tuple(perms.shape) != (update_epochs, rows) or perms.dtype != torch.int64
                                  or perms.device != self.device or not perms.is_contiguous()):
            raise ValueError("perms must be a contiguous int64 [update_epochs, R] tensor on the policy's device")
        out = []
        for e in range(int(update_epochs)):
            b_inds = perms[e] if perms is not None else torch.randperm(rows, device=self.device)
            for start in range(0, rows, mb):
                out.append(self.ppo_minibatch(obs, actions, log_prob, value, advantages, returns,
                                              b_inds[start:start + mb], state, **kw))
        return torch.stack(out)

    # --------------------------------------------------------- PPO advantages
    def compute_advantages(self, buffers: dict, advantages: torch.Tensor, returns: torch.Tensor, value_norm,
                           obs_norm=None, gamma: float = 0.998, gae_lambda: float = 0.95) -> torch.Tensor:
        """compute_advantages (scripts/ppo.py:144-177) on the device,
        bb_policy_advantages (at 184 to 424 inputs bb_policy_advantages_wide): from
        the buffers of a rollout (obs [K, W, in_dim],
        value / reward / done [K, W], next_value [W]) the GAE recursion on the
        un-normalised values (agent.py:31-34 with clamp 5; the last step's
        non-terminal flag is 1 - done[K-1], as ppo.py:157 has it), then
        obs_norm.update(obs rows), value_norm.update(values),
        value_norm.update(returns) in this order (agent.py:41-50, the float64
        buffers updated in place), then advantages [K, W] = (A - mean) / (std +
        1e-8) and returns [K, W] = the updated value_norm's clamped normalisation
        of A + values.  value_norm / obs_norm: any objects with float64 tensors
        mean [dim], var [dim], count [] on the policy's device (dim 1 / in_dim; a
        RunningMeanStd, a RunningStats); obs_norm=None: the agent's own.
        buffers["value"] is left as it is: ppo.py:175's `values[:] = ...` writes
        to a temporary, and ppo_grad() takes the policy's own normalised values.
        The packed weights still hold the old observation statistics: call
        refresh() afterwards, as after an optimizer step.  Returns a float32 [4]
        tensor on the device: mean and unbiased std of A before normalisation,
        value_norm's new mean and var (no host synchronisation; torch's current
        stream)."""
        dev, f32, f64, width = self.device, torch.float32, torch.float64, self.in_dim
        obs = buffers.get("obs")
        if (obs is None or obs.dim() != 3 or obs.shape[2] != width or obs.dtype != f32 or not obs.is_contiguous()
                or obs.device != dev):
            raise ValueError(f"buffers['obs'] must be a contiguous float32 [K, W, {width}] tensor on the policy's "
                             "device")
        K, W = obs.shape[0], obs.shape[1]
        if K * W < 2:
            raise ValueError("compute_advantages needs at least 2 rows (the unbiased variance of one is undefined)")
        named = {k: buffers.get(k) for k in ("value", "reward", "done")}
        named.update(advantages=advantages, returns=returns)
        for k, t in named.items():
            if t is None or tuple(t.shape) != (K, W) or t.dtype != f32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{k} must be a contiguous float32 [{K}, {W}] tensor on the policy's device")
        nv = buffers.get("next_value")
        if nv is None or tuple(nv.shape) != (W,) or nv.dtype != f32 or not nv.is_contiguous() or nv.device != dev:
            raise ValueError(f"buffers['next_value'] must be a contiguous float32 [{W}] tensor on the policy's device")
        if obs_norm is None:
            obs_norm = self.agent.obs_norm
        stats = []
        for name, norm, dim in (("value_norm", value_norm, 1), ("obs_norm", obs_norm, width)):
            for field, shape in (("mean", (dim,)), ("var", (dim,)), ("count", ())):
                t = getattr(norm, field, None)
                if (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != f64
                        or not t.is_contiguous() or t.device != dev):
                    raise ValueError(f"{name}.{field} must be a float64 {shape} tensor on the policy's device")
            stats.append(_lib.RunningStatsPtrs(norm.mean.data_ptr(), norm.var.data_ptr(), norm.count.data_ptr()))
        lib = _lib.load()
        cuda = dev.type == "cuda"
        wide = () if width == IN else (width,)
        entry = lib.bb_policy_advantages if width == IN else lib.bb_policy_advantages_wide
        query = (lib.bb_policy_advantages_workspace_bytes if width == IN
                 else lib.bb_policy_advantages_wide_workspace_bytes)
        need = query(*wide, K, W) if cuda else 0
        if getattr(self, "_adv_ws", None) is None or self._adv_ws.numel() * 8 < need:
            self._adv_ws = torch.empty((max(need, 8) // 8,), dtype=f64, device=dev)
        out4 = torch.empty((4,), dtype=f32, device=dev)
        batch = _lib.AdvBatch(obs.data_ptr(), named["value"].data_ptr(), named["reward"].data_ptr(),
                              named["done"].data_ptr(), nv.data_ptr(), advantages.data_ptr(), returns.data_ptr(), K, W)
        _lib.check(entry(
            *wide, int(ExecMode.CUDA if cuda else ExecMode.CPU), dev.index if dev.index is not None else -1,
            ctypes.byref(batch), ctypes.byref(stats[0]), ctypes.byref(stats[1]), float(gamma), float(gae_lambda),
            ctypes.c_void_p(out4.data_ptr()), ctypes.c_void_p(self._adv_ws.data_ptr() if cuda else None), need,
            self._stream()), "policy_advantages")
        return out4

    # ------------------------------------------------------------ PPO rollout
    ROLLOUT_KEYS = ("obs", "actions", "log_prob", "value", "reward", "done", "next_value")

    def rollout_buffers(self, sim, n: int) -> dict:
        """Zeroed outputs of rollout() on the simulator's device -- the storage of
        scripts/buffers.py:4-11 for n steps of the trainee (obs [n, W, 128],
        actions int32 [n, W, 6], log_prob / value / reward / done [n, W]) and
        next_value [W] (ppo.py:136-137)."""
        W, dev, f32 = sim.num_worlds, sim.device, torch.float32
        return {"obs": torch.zeros((n, W, IN), dtype=f32, device=dev),
                "actions": torch.zeros((n, W, 6), dtype=torch.int32, device=dev),
                "log_prob": torch.zeros((n, W), dtype=f32, device=dev),
                "value": torch.zeros((n, W), dtype=f32, device=dev),
                "reward": torch.zeros((n, W), dtype=f32, device=dev),
                "done": torch.zeros((n, W), dtype=f32, device=dev),
                "next_value": torch.zeros((W,), dtype=f32, device=dev)}

    def rollout(self, sim, n: int, buffers: dict, trainee: int = 0, stochastic: bool = True, seed: int = 0,
                step0: int = 0, opponent: "FusedPolicy" = None, per_step: bool = False, time_kernels: bool = False):
        """PPO's rollout loop (scripts/ppo.py:61-141) on the device, bb_rollout_policy:
        n x (this policy acts for agent `trainee` of every world; [the frozen
        `opponent` acts for the other agent, env.py:127-143]; step) with the
        buffer stores of ppo.py:129-134 and next_value = evaluate(last obs).
        Bit for bit n x (act(); [opponent.act()]; sim.step()) with the same reads.
        Any entry of `buffers` may be None (not recorded).  On gfx950 (2 agents)
        one fused launch runs every step, with the opponent's network in it
        when there is one, at every world count (nothing of the opponent is
        recorded); per_step=True forces a policy launch per acting agent + a
        step launch per step.  Returns
        the elapsed device ms when time_kernels."""
        self._require_128("rollout")
        W = sim.num_worlds
        shapes = {"obs": ((n, W, IN), torch.float32), "actions": ((n, W, 6), torch.int32),
                  "log_prob": ((n, W), torch.float32), "value": ((n, W), torch.float32),
                  "reward": ((n, W), torch.float32), "done": ((n, W), torch.float32),
                  "next_value": ((W,), torch.float32)}
        ptrs = {}
        for k in self.ROLLOUT_KEYS:
            t = buffers.get(k)
            if t is not None:
                shp, dt = shapes[k]
                if tuple(t.shape) != shp or t.dtype != dt or not t.is_contiguous() or t.device != sim.device:
                    raise ValueError(f"rollout buffer {k!r} must be a contiguous {dt} {shp} tensor on the "
                                     "simulator's device")
            ptrs[k] = None if t is None else t.data_ptr()
        if (buffers.get("reward") is None) != (buffers.get("done") is None):
            raise ValueError("reward and done are recorded together")
        if sim.device != self.device or (opponent is not None and opponent.device != self.device):
            raise ValueError("policy, opponent and simulator must share a device")
        out = _lib.PolicyRolloutBuffers(**ptrs)
        ms = ctypes.c_float(0.0)
        _lib.check(_lib.load().bb_rollout_policy(
            sim._h, ctypes.byref(self._w), ctypes.byref(opponent._w) if opponent is not None else None, int(n),
            int(trainee), 1 if stochastic else 0, int(seed) & 0xFFFFFFFF, int(step0) & 0xFFFFFFFF,
            ctypes.byref(out), _lib.ROLLOUT_PER_STEP if per_step else 0, sim._stream(),
            ctypes.byref(ms) if time_kernels else None), "rollout_policy")
        return ms.value if time_kernels else None
