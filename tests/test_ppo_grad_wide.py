"""Fused PPO loss + gradient at 184, 264, 344 and 424 inputs
(FusedPolicy.ppo_grad_wide, bb_policy_ppo_grad_wide) against update_policy's
loss in torch float64 with autograd: tests/test_ppo_grad.py's method, loss,
cases and bound (per tensor and loss max |new - f64| <= 4 x max |torch f32
autograd - f64|, floored at 2^-20 |ref|_inf) on the wide RefAgent of
tests/test_policy_wide.py.  Precondition, from the float64 reference alone: no
pre-ReLU LayerNorm output of the 100 rows within 1e-5 of 0 (SEED: seeds for
which it holds at every width).

Grid rules (csrc/bb_policy_grad_wide.hip): pass 1 has 8 waves x 256 workgroups,
pass 2 has 8 / 4 waves per column slab x 256 at 184 / 424 inputs; "big" =
2 048 tiles + 21 rows is the smallest M at which a wave of either pass takes a
second tile, the last tile partial.  It runs at the two outer widths only.
"""
import copy
import ctypes
import functools

import pytest
import torch

from madrona_basketball_amd import _lib
from madrona_basketball_amd.policy import BUCKETS, FusedPolicy, make_agent
from tests.test_policy_wide import RefAgent
from tests.test_ppo_grad import BATCH, BIG, CASES, CLIP, ENT, VF, R, params, torch_loss

WIDTHS = (184, 264, 344, 424)
SEED = 1
assert BIG == 2048 * 16 + 21
GRID = [(w, c) for w in WIDTHS for c in CASES if c != "big" or w in (184, 424)]


@functools.lru_cache(None)
def base(width):
    """The agent, its packed normaliser and the 100 buffer rows (CPU), as test_ppo_grad.base() builds them."""
    g = torch.Generator().manual_seed(SEED)
    agent = RefAgent(width, seed=11)
    pol = FusedPolicy.from_agent(agent)
    norm = (pol._tensors["obs_mean"], pol._tensors["obs_inv"])
    obs = torch.randn(R, width, generator=g) * 8
    obs[torch.rand(R, width, generator=g) < 0.1] = 0.0
    d = {"obs": obs, "actions": torch.stack([torch.randint(0, nb, (R,), generator=g) for nb in BUCKETS], 1).int()}
    d.update(log_prob=torch.zeros(R), value=torch.zeros(R), adv=torch.zeros(R), ret=torch.zeros(R))
    i = torch.arange(R)
    with torch.no_grad():
        _, pre, lp_ref, v_ref = torch_loss(copy.deepcopy(agent).double(), norm, d, None)
    assert min(y.abs().min().item() for y in pre) > 1e-5  # the precondition, from the reference alone
    d["log_prob"] = (lp_ref - torch.log(torch.tensor([0.7, 0.9, 1.0, 1.1, 1.3], dtype=torch.float64)[i % 5])).float()
    d["adv"] = (0.5 + torch.rand(R, generator=g)) * (1 - 2 * (i % 2)).float()
    d["value"] = (v_ref - torch.tensor([-0.5, -0.1, 0.1, 0.5], dtype=torch.float64)[i % 4]).float()
    d["ret"] = (v_ref + torch.tensor([-1.0, 0.3, 1.0], dtype=torch.float64)[i % 3]).float()
    return agent, norm, d


@functools.lru_cache(None)
def reference(width, case):
    """(float64, float32) torch autograd results of a case: [12 grads + loss4] each."""
    agent, norm, d = base(width)
    out = []
    for dt in (torch.float64, torch.float32):
        ag = copy.deepcopy(agent).to(dt)
        loss = torch_loss(ag, norm, d, CASES[case]())[0]
        loss[0].backward()
        out.append([p.grad.double() for p in params(ag)] + [loss.detach().double()])
    return out


@pytest.mark.parametrize("width,case", GRID)
@pytest.mark.parametrize("mode", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_ppo_grad_wide_vs_float64(native_lib, mode, width, case):
    agent, _, d = base(width)
    agent = copy.deepcopy(agent).to(mode)
    pol = FusedPolicy.from_agent(agent)
    idx = CASES[case]()
    args = [d[k].to(mode) for k in BATCH] + [None if idx is None else idx.to(mode)]
    runs = []
    for _ in range(2):
        loss4 = pol.ppo_grad_wide(*args, clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)
        runs.append([p.grad.clone() for p in params(agent)] + [loss4])
    for a, b in zip(*runs):  # the same bits on every call
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not pol.head_grad[0][20:].any() and not pol.head_grad[1][20:].any()
    f64, f32 = reference(width, case)
    for k, (new, ref, t32) in enumerate(zip(runs[0], f64, f32)):
        dev, own = (new.cpu().double() - ref).abs().max().item(), (t32 - ref).abs().max().item()
        bound = max(4 * own, 2.0 ** -20 * ref.abs().max().item())
        print(f"{mode} {width} {case} tensor {k}: dev {dev:.3e} torch-f32 {own:.3e} ratio {dev / max(own, 1e-300):.2f}")
        assert dev <= bound, (k, dev, own, bound)


def test_ppo_grad_wide_interface(native_lib):
    agent, _, d = base(184)
    pol = FusedPolicy.from_agent(copy.deepcopy(agent))
    args = [d[k] for k in BATCH]
    with pytest.raises(ValueError, match="use ppo_grad"):
        FusedPolicy.from_agent(make_agent(1)).ppo_grad_wide(*args)
    with pytest.raises(ValueError, match="184"):
        pol.ppo_grad_wide(base(264)[2]["obs"], *args[1:])
    # the C entry: a workspace one byte short (device mode) and another width are errors, nothing is launched
    L, m = native_lib, 64
    need = L.bb_policy_ppo_grad_wide_workspace_bytes(184, m)
    assert need > 0 and L.bb_policy_ppo_grad_wide_workspace_bytes(200, m) == 0
    ws, loss4, sink = torch.zeros(need // 4), torch.zeros(4), torch.zeros(32 * 184)
    batch = _lib.PpoBatch(*[t.data_ptr() for t in args], None, R, m)
    coef, grads = _lib.PpoCoef(CLIP, VF, ENT), _lib.PolicyGrads(*[sink.data_ptr()] * 10)
    call = lambda in_dim, nbytes: L.bb_policy_ppo_grad_wide(
        ctypes.byref(pol._w), in_dim, _lib.EXEC_CUDA, 0, ctypes.byref(batch), ctypes.byref(coef), ctypes.byref(grads),
        loss4.data_ptr(), ws.data_ptr(), nbytes, None)
    assert call(184, need - 1) < 0 and b"workspace" in L.bb_last_error()
    assert call(200, need) < 0 and b"in_dim" in L.bb_last_error()
