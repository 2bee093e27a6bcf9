"""Fused policy inference at the observation widths of 4, 6, 8 and 10 agents
(bb_policy_forward_wide, csrc/bb_policy_wide.hip): 184, 264, 344, 424 inputs.

The checker is a plain torch restatement of the reference's Agent at
input_dim = IN (tests/test_policy.py has the 128-wide one), evaluated in
float64 as the reference and in float32 as the yardstick: value / log-prob may
deviate from float64 by at most 4 x the float32 torch forward's own maximum
deviation on the same rows (a different, equally valid summation order over up
to 424 terms), floor 2^-20 max|x|.  Measured host / torch-f32 deviation ratios
(W = 512, one agent column): DESIGN.md 15.
"""
import copy
import ctypes
import functools

import pytest
import torch
import torch.nn as nn

from madrona_basketball_amd import ExecMode, _lib
from madrona_basketball_amd.policy import BUCKETS, FusedPolicy, make_agent
from tests.helpers import make_sim

WIDTH = {4: 184, 6: 264, 8: 344, 10: 424}
AGENTS = sorted(WIDTH)
HI = torch.tensor(BUCKETS)


class RefAgent(nn.Module):  # scripts/agent.py:19-38, 108-154 at num_channels 32, num_layers 2
    def __init__(self, in_dim, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.action_buckets = list(BUCKETS)
        self.backbone = nn.Sequential(nn.Linear(in_dim, 32), nn.LayerNorm(32), nn.ReLU(),
                                      nn.Linear(32, 32), nn.LayerNorm(32), nn.ReLU())
        self.actor, self.critic = nn.Linear(32, 19), nn.Linear(32, 1)
        self.obs_norm = nn.Module()
        self.obs_norm.epsilon = 1e-5
        self.obs_norm.register_buffer("mean", torch.randn(in_dim, generator=g, dtype=torch.float64) * 3)
        self.obs_norm.register_buffer("var", torch.rand(in_dim, generator=g, dtype=torch.float64) * 20 + 0.01)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() > 1 else 0.3))

    def logits_value(self, obs):
        n = self.obs_norm
        x = torch.clamp((obs - n.mean.to(obs.dtype)) * torch.rsqrt(n.var.to(obs.dtype) + n.epsilon), -5.0, 5.0)
        x = self.backbone(x)
        return self.actor(x), self.critic(x).squeeze(-1)


def scored(logits, acts):
    """Summed log-softmax of `acts` ([R, 6]; None: the per-bucket argmax)."""
    out, lp, o = [], 0.0, 0
    for b, nb in enumerate(BUCKETS):
        ls = torch.log_softmax(logits[:, o:o + nb], -1)
        a = ls.argmax(-1) if acts is None else acts[:, b].long()
        out.append(a)
        lp = lp + ls.gather(1, a[:, None])[:, 0]
        o += nb
    return torch.stack(out, 1), lp


def margin_ok(logits):
    ok, o = torch.ones(logits.shape[0], dtype=torch.bool), 0
    for nb in BUCKETS:
        top = torch.topk(logits[:, o:o + nb], 2, dim=-1).values
        ok &= (top[:, 0] - top[:, 1]) > 1e-4
        o += nb
    return ok


@torch.no_grad()
def check_vs_float64(ref, obs, acts, lp, v, sampled=False):
    """obs, acts, lp, v on the CPU; ref a float32 RefAgent (any device)."""
    ref = copy.deepcopy(ref).cpu()
    l32, v32 = ref.logits_value(obs)
    l64, v64 = ref.double().logits_value(obs.double())
    a64, lp64 = scored(l64, acts if sampled else None)
    _, lp32 = scored(l32, a64)
    for name, got, r32, r64 in (("value", v, v32, v64), ("log_prob", lp, lp32, lp64)):
        yard = (r32.double() - r64).abs().max().item()
        err = (got.double() - r64).abs().max().item()
        print(f"IN {obs.shape[1]} {name}: |host - f64| {err:.3e}, |torch f32 - f64| {yard:.3e}, ratio {err / yard:.2f}")
        assert err <= max(4 * yard, 2.0 ** -20 * r64.abs().max().item()), (name, err, yard)
    if not sampled:
        ok = margin_ok(l64)
        assert ok.float().mean() > 0.95
        assert torch.equal(acts[ok].long(), a64[ok])


@functools.lru_cache(maxsize=None)
def sim_obs(mode, worlds, n):
    sim = make_sim(mode, worlds, num_agents=n, per_world_rng=True)
    sim.step_n(100, random_actions=True, action_seed=12)
    return sim.observations_tensor().to_torch().clone()


@pytest.mark.parametrize("n", AGENTS)
def test_host_wide_policy_vs_float64(native_lib, n):
    obs = sim_obs(ExecMode.CPU, 512, n)[:, 1]  # one agent column: row stride N * OW
    ref = RefAgent(WIDTH[n], seed=3 + n)
    pol = FusedPolicy.from_agent(ref)
    assert pol.in_dim == WIDTH[n]
    acts, lp, v = pol(obs, stochastic=False)
    check_vs_float64(ref, obs, acts, lp, v)
    a1, lp1, v1 = pol(obs, stochastic=True, seed=7, step=1)
    assert torch.all((a1 >= 0) & (a1 < HI)) and torch.equal(v1, v)
    check_vs_float64(ref, obs, a1, lp1, v1, sampled=True)
    assert not torch.equal(a1, pol(obs, stochastic=True, seed=7, step=2)[0])  # the step is part of the key


def equal_bits(pol_g, pol_h, obs, stochastic):
    ag, lpg, vg = pol_g(obs, stochastic=stochastic, seed=3, step=11)
    ah, lph, vh = pol_h(obs.cpu(), stochastic=stochastic, seed=3, step=11)
    assert torch.equal(ag.cpu(), ah)
    assert torch.equal(lpg.cpu().view(torch.int32), lph.view(torch.int32))
    assert torch.equal(vg.cpu().view(torch.int32), vh.view(torch.int32))
    return ag.cpu(), lpg.cpu(), vg.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("n", AGENTS)
def test_gpu_wide_policy_equals_host(native_lib, n, stochastic):
    obs = sim_obs(ExecMode.CUDA, 2048, n)
    ref = RefAgent(WIDTH[n], seed=9 + n).cuda()
    pol_g = FusedPolicy.from_agent(ref)
    pol_h = pol_g.to("cpu")
    rows = obs.view(-1, WIDTH[n])
    out = equal_bits(pol_g, pol_h, rows, stochastic)       # every agent's rows, contiguous
    for r in (1, 16, 17):                                  # the tile edge, a part-filled last tile
        equal_bits(pol_g, pol_h, rows[100:100 + r], stochastic)
    equal_bits(pol_g, pol_h, obs[:, n - 1], stochastic)    # one agent column, strided
    if not stochastic:
        check_vs_float64(ref, rows.cpu(), *out)


@pytest.mark.gpu
@pytest.mark.parametrize("n", AGENTS)
def test_gpu_wide_policy_second_tile_per_wave(native_lib, n):
    """More 16-row tiles than one round of the grid (12 waves x 256 workgroups =
    3 072): waves take a second tile with its first chunks loaded under the
    first tile's tail.  Argmax (no row keys), so the host runs the first and
    the last 1 024 rows only: first-round tiles with the prefetch live, and
    the second round."""
    worlds = -(-(3072 + 64) * 16 // n)
    obs = sim_obs(ExecMode.CUDA, worlds, n).view(-1, WIDTH[n])
    assert obs.shape[0] >= 3072 * 16 + 1024
    pol_g = FusedPolicy.from_agent(RefAgent(WIDTH[n], seed=4).cuda())
    pol_h = pol_g.to("cpu")
    ag, lpg, vg = (t.cpu() for t in pol_g(obs, stochastic=False))
    for sl in (slice(0, 1024), slice(obs.shape[0] - 1024, obs.shape[0])):
        ah, lph, vh = pol_h(obs[sl].cpu(), stochastic=False)
        assert torch.equal(ag[sl], ah)
        assert torch.equal(lpg[sl].view(torch.int32), lph.view(torch.int32))
        assert torch.equal(vg[sl].view(torch.int32), vh.view(torch.int32))


@pytest.mark.gpu
def test_gpu_wide_policy_act_all_in_the_loop(native_lib):
    pol_g = FusedPolicy.from_agent(RefAgent(184, seed=2).cuda())
    pol_h = pol_g.to("cpu")
    g = make_sim(ExecMode.CUDA, 1024, num_agents=4, per_world_rng=True)
    h = make_sim(ExecMode.CPU, 1024, num_agents=4, per_world_rng=True)
    for t in range(60):
        pol_g.act_all(g, stochastic=True, seed=1, step=t)
        pol_h.act_all(h, stochastic=True, seed=1, step=t)
        g.step()
        h.step()
    torch.cuda.synchronize()
    for name in g._views:
        assert torch.equal(g._views[name].cpu(), h._views[name]), name


def test_wide_policy_interface(native_lib):
    pol = FusedPolicy.from_agent(make_agent(1, input_dim=184))
    with pytest.raises(ValueError, match="128-wide"):
        pol.rollout(None, 1, {})
    with pytest.raises(ValueError, match="128-wide"):
        pol.ppo_grad(*[None] * 6)
    with pytest.raises(ValueError):
        FusedPolicy.from_agent(make_agent(1, input_dim=200))
    with pytest.raises(ValueError, match="cannot act"):
        pol.act_all(make_sim(ExecMode.CPU, 8, num_agents=6))
    # a 128-wide policy still goes through bb_policy_forward: the same bits as a direct call
    p128 = FusedPolicy.from_agent(make_agent(2))
    obs = sim_obs(ExecMode.CPU, 64, 2)[:, 0]
    a, lp, v = p128(obs, stochastic=True, seed=5, step=9)
    a2, lp2, v2 = torch.empty_like(a), torch.empty_like(lp), torch.empty_like(v)
    vp = ctypes.c_void_p
    _lib.check(native_lib.bb_policy_forward(ctypes.byref(p128._w), 0, -1, vp(obs.data_ptr()), 64, obs.stride(0),
                                            vp(a2.data_ptr()), 6, vp(lp2.data_ptr()), vp(v2.data_ptr()), 1, 5, 9,
                                            vp(None)), "policy_forward")
    assert torch.equal(a, a2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(v, v2)
