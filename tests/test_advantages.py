"""Fused GAE + normaliser updates + advantage normalisation
(FusedPolicy.compute_advantages, bb_policy_advantages) against compute_advantages
(scripts/ppo.py:144-177) over RunningMeanStd (scripts/agent.py:28-50) written in
torch float64 throughout.

Bound (DESIGN.md section 12's), per output tensor -- advantages, returns, both
normalisers' mean and var, the [4] result: max |new - f64| <= max(4 x max |torch
f32 literal - f64|, 2^-20 |ref|_inf); both counts exact.  Preconditions, from
the float64 reference alone: no |value| within 1e-3 of 5, no normalised return
within 1e-4 of +-5, sigma > 1e-3.

Grid rule of the launch (csrc/bb_advantages.h adv_grid): GAE role min(64,
ceil(W / 256)) workgroups of 256 lanes, one world per lane; observation role
min(512, ceil(K W / 64)) workgroups of 4 waves x 16 rows; both grid-stride.
BIG = (2, 64 x 256 + 64 + 5): a second GAE pass of one full and one partial
wave, and 2 W = 512 x 64 + 138 rows, a second observation pass of 8 full
16-row waves and one of 10 rows.
"""
import ctypes
import functools

import pytest
import torch

from madrona_basketball_amd import _lib
from madrona_basketball_amd.policy import FusedPolicy, RunningStats, make_agent

GAMMA, LAM = 0.998, 0.95
SHAPES = {"1x2": (1, 2), "2x1": (2, 1), "3x65": (3, 65), "32x100": (32, 100), "big": (2, 64 * 256 + 64 + 5)}
OUT = ("advantages", "returns", "vn.mean", "vn.var", "on.mean", "on.var", "out4", "vn.count", "on.count")


@functools.lru_cache(None)
def inputs(shape):
    """Seeded buffers and normaliser states (CPU): dones at t = K-1 and t = 0, values beyond +-5,
    rewards that end an episode and put its return beyond +-5, observation columns with means of
    order 10 and zero columns, normalisers away from their initial state with counts in the thousands."""
    K, W = SHAPES[shape]
    g = torch.Generator().manual_seed(5)
    value = torch.randn(K, W, generator=g) * 0.8
    value.view(-1)[::13] = 6.5 * (1 - 2 * (torch.arange(0, K * W, 13) % 2)).float()
    done = (torch.rand(K, W, generator=g) < 0.1).float()
    done[K - 1, 0], done[0, W - 1] = 1.0, 1.0
    reward = torch.randn(K, W, generator=g) * 0.3 + 60.0 * done * (1 - 2 * (torch.rand(K, W, generator=g) < 0.3).float())
    obs = torch.randn(K, W, 128, generator=g) * (torch.rand(128, generator=g) * 8) + torch.randn(128, generator=g) * 10
    obs[..., ::9] = 0.0
    vn = (torch.tensor([0.7], dtype=torch.float64), torch.tensor([2.3], dtype=torch.float64),
          torch.tensor(3000.0, dtype=torch.float64))
    on = (torch.randn(128, generator=g, dtype=torch.float64) * 3, torch.rand(128, generator=g, dtype=torch.float64) * 20
          + 0.01, torch.tensor(5000.0, dtype=torch.float64))
    return {"obs": obs, "value": value, "reward": reward, "done": done,
            "next_value": torch.randn(W, generator=g) * 0.8, "vn": vn, "on": on}


def literal(d, dt):
    """compute_advantages as the reference writes it, the buffers held in dtype dt."""
    vn, on = [t.clone() for t in d["vn"]], [t.clone() for t in d["on"]]

    def forward(st, x, unnorm=False):  # agent.py:28-38 with clamp 5
        mean, var = st[0].to(dt), st[1].to(dt) + 1e-5
        if unnorm:
            return mean + torch.sqrt(var) * torch.clamp(x, -5.0, 5.0)
        return (x - mean) * torch.rsqrt(var)

    def update(st, x):  # agent.py:41-50
        var, mean = torch.var_mean(x, dim=0, unbiased=True)
        count = x.size(0)
        count_ = count + st[2]
        delta = mean - st[0]
        m = st[1] * st[2] + var * count + delta ** 2 * st[2] * count / count_
        st[0], st[1], st[2] = st[0] + delta * count / count_, m / count_, count_

    rewards, not_dones = d["reward"].to(dt), 1 - d["done"].to(dt)
    values, next_value = forward(vn, d["value"].to(dt), True), forward(vn, d["next_value"].to(dt), True)
    K = rewards.shape[0]
    advantages, last = torch.zeros_like(rewards), 0.0
    for t in reversed(range(K)):
        nnt, nxt = (not_dones[t], next_value) if t == K - 1 else (not_dones[t + 1], values[t + 1])
        delta = rewards[t] + GAMMA * nxt * nnt - values[t]
        advantages[t] = last = delta + GAMMA * LAM * nnt * last
    returns = advantages + values
    update(on, d["obs"].to(dt).view(-1, 128))
    update(vn, values.view(-1, 1))
    update(vn, returns.view(-1, 1))
    mu, sigma = advantages.mean(), advantages.std()
    advantages = (advantages - mu) / (sigma + 1e-8)
    raw = forward(vn, returns)
    out4 = torch.stack([mu.double(), sigma.double(), vn[0][0], vn[1][0]])
    return [advantages, torch.clamp(raw, -5.0, 5.0), vn[0], vn[1], on[0], on[1], out4, vn[2], on[2]], raw, sigma


@functools.lru_cache(None)
def reference(shape):
    """(float64, float32) results of a shape; the preconditions, from the float64 one alone."""
    d = inputs(shape)
    f64, raw, sigma = literal(d, torch.float64)
    assert ((d["value"].abs() - 5).abs() > 1e-3).all() and ((raw.abs() - 5).abs() > 1e-4).all() and sigma > 1e-3
    assert (d["value"].abs() > 5).any() and (raw.abs() > 5).any()
    return f64, [t.double() for t in literal(d, torch.float32)[0]]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("mode", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_advantages_vs_float64(native_lib, mode, shape):
    d = inputs(shape)
    f64, f32 = reference(shape)  # on the CPU, before anything goes to the device
    pol = FusedPolicy.from_agent(make_agent(0).to(mode))
    buf = {k: d[k].to(mode) for k in ("obs", "value", "reward", "done", "next_value")}
    runs = []
    for _ in range(2):
        vn, on = RunningStats(1, mode), RunningStats(128, mode)
        for st, src in ((vn, d["vn"]), (on, d["on"])):
            st.mean.copy_(src[0]); st.var.copy_(src[1]); st.count.copy_(src[2])
        adv, ret = torch.empty_like(buf["value"]), torch.empty_like(buf["value"])
        out4 = pol.compute_advantages(buf, adv, ret, vn, on, GAMMA, LAM)
        runs.append([t.cpu() for t in (adv, ret, vn.mean, vn.var, on.mean, on.var, out4, vn.count, on.count)])
    assert torch.equal(buf["value"].cpu().view(torch.int32), d["value"].view(torch.int32))
    for a, b in zip(*runs):  # the same bits on every call
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    for name, new, ref, t32 in zip(OUT, runs[0], f64, f32):
        if name.endswith("count"):
            assert new.item() == ref.item()
            continue
        dev, own = (new.double() - ref).abs().max().item(), (t32 - ref).abs().max().item()
        bound = max(4 * own, 2.0 ** -20 * ref.abs().max().item())
        print(f"{mode} {shape} {name}: dev {dev:.3e} torch-f32 {own:.3e} ratio {dev / max(own, 1e-300):.2f}")
        assert dev <= bound, (name, dev, own, bound)


def test_advantages_bad_arguments(native_lib):
    d = inputs("3x65")
    pol = FusedPolicy.from_agent(make_agent(0))
    buf = {k: d[k] for k in ("obs", "value", "reward", "done", "next_value")}
    adv, ret, vn, on = torch.empty(3, 65), torch.empty(3, 65), RunningStats(1), RunningStats(128)
    for bad in (dict(advantages=adv.double()), dict(returns=ret[:2]), dict(obs_norm=None),  # make_agent's: no count
                dict(buffers={**buf, "done": buf["done"].t()}),
                dict(buffers={k: v[:1, :1] if v.dim() > 1 else v[:1] for k, v in buf.items()}, advantages=adv[:1, :1],
                     returns=ret[:1, :1])):
        with pytest.raises(ValueError):
            pol.compute_advantages(**{**dict(buffers=buf, advantages=adv, returns=ret, value_norm=vn, obs_norm=on), **bad})
    # the C entry: NULL, misaligned and short-workspace calls are errors, nothing is launched
    L = native_lib
    need = L.bb_policy_advantages_workspace_bytes(3, 65)
    assert need > 0 and L.bb_policy_advantages_workspace_bytes(1, 1) > 0
    ws, out4 = torch.zeros(need // 8, dtype=torch.float64), torch.zeros(4)
    stats = [_lib.RunningStatsPtrs(s.mean.data_ptr(), s.var.data_ptr(), s.count.data_ptr()) for s in (vn, on)]

    def call(mode=_lib.EXEC_CUDA, nbytes=need, steps=3, worlds=65, **ptr):
        p = {**{k: v.data_ptr() for k, v in buf.items()}, "advantages": adv.data_ptr(), "returns": ret.data_ptr(), **ptr}
        batch = _lib.AdvBatch(p["obs"], p["value"], p["reward"], p["done"], p["next_value"], p["advantages"],
                              p["returns"], steps, worlds)
        return L.bb_policy_advantages(mode, 0, ctypes.byref(batch), ctypes.byref(stats[0]), ctypes.byref(stats[1]),
                                      GAMMA, LAM, out4.data_ptr(), ws.data_ptr(), nbytes, None)
    assert call(nbytes=need - 1) < 0 and b"workspace" in L.bb_last_error()
    assert call(mode=_lib.EXEC_CPU, reward=None) < 0 and b"NULL" in L.bb_last_error()
    assert call(mode=_lib.EXEC_CPU, obs=buf["obs"].data_ptr() + 4) < 0 and b"aligned" in L.bb_last_error()
    assert call(mode=_lib.EXEC_CPU, steps=1, worlds=1) < 0 and call(mode=7) < 0
    stats[0].var = vn.var.data_ptr() + 4
    assert call(mode=_lib.EXEC_CPU) < 0 and b"8-byte" in L.bb_last_error()
