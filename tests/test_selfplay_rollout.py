"""Self-play in the fused PPO rollout (k_rollout_selfplay: bb_rollout_policy with
a frozen opponent, scripts/env.py:104-143, in one launch) == the per-step
launches and the host executor, every record and every column, bit for bit."""
import pytest
import torch

from madrona_basketball_amd import ExecMode, _lib
from madrona_basketball_amd.policy import FusedPolicy, make_agent
from tests.helpers import make_sim
from tests.test_policy_rollout import assert_same

HOST, FUSED_ROLLOUT, PER_STEP = 0, 1, 3  # BB_PPO_PATH_*


def test_selfplay_path_on_the_host_executor(native_lib):
    assert native_lib.bb_rollout_policy_path(make_sim(ExecMode.CPU, 64)._h, 1, 0) == HOST


@pytest.mark.gpu
def test_gpu_selfplay_takes_the_fused_rollout(native_lib):
    sim = make_sim(ExecMode.CUDA, 8192)
    assert native_lib.bb_rollout_policy_path(sim._h, 1, 0) == FUSED_ROLLOUT
    assert native_lib.bb_rollout_policy_path(sim._h, 1, _lib.ROLLOUT_PER_STEP) == PER_STEP
    with _lib.diag(ppo_fused_max_worlds=0):
        assert native_lib.bb_rollout_policy_path(sim._h, 1, 0) == PER_STEP


def fused_vs_per_step(W, n, trainee, stochastic, opp_seed=4, opp_gain=1.0):
    sims = [make_sim(ExecMode.CUDA, W, per_world_rng=True) for _ in range(2)]
    for s in sims:
        s.step_n(9, random_actions=True, action_seed=321, step0=0)
    assert _lib.load().bb_rollout_policy_path(sims[0]._h, 1, 0) == FUSED_ROLLOUT
    pol = FusedPolicy.from_agent(make_agent(3).cuda())
    opp_agent = make_agent(opp_seed)
    opp_agent.actor.weight.data.mul_(opp_gain)  # (make_agent's heads have gain 0.01: logits near 0)
    opp = FusedPolicy.from_agent(opp_agent.cuda())
    bufs = [pol.rollout_buffers(s, n) for s in sims]
    for s, b, per_step in zip(sims, bufs, (False, True)):
        pol.rollout(s, n, b, trainee=trainee, stochastic=stochastic, seed=11, step0=5, opponent=opp, per_step=per_step)
    torch.cuda.synchronize()
    assert_same(bufs[0], bufs[1])
    for name in sims[0]._views:
        assert torch.equal(sims[0]._views[name], sims[1]._views[name]), name
    return bufs[0], sims[0]


@pytest.mark.gpu
@pytest.mark.parametrize("W,n,trainee,stochastic,ow", [  # ow: the ppo_opp_waves override (-1: the launcher's rule)
    (33, 3, 0, True, -1),      # one full workgroup plus one world
    (64, 3, 1, False, -1),     # an argmax trainee beside the sampling opponent
    (1000, 20, 0, True, 1),    # a partial last workgroup, one opponent wave (4 waves, whole register file)
    (1000, 20, 0, True, 2),    # ... two opponent waves
    (16384, 6, 1, True, -1),   # the bound: two workgroups per CU
    (1000, 640, 0, True, -1),  # across the 620-step clock expiry and the in-launch reset
])
def test_gpu_selfplay_rollout_equals_per_step_launches(native_lib, W, n, trainee, stochastic, ow):
    with _lib.diag(ppo_opp_waves=ow):
        bufs, _ = fused_vs_per_step(W, n, trainee, stochastic)
    if n > 620:
        assert (bufs["done"] == 1).any(dim=0).all()  # every world was reset inside the launch


@pytest.mark.gpu
def test_gpu_selfplay_rollout_equals_host_executor(native_lib):
    outs = []
    for mode, dev in ((ExecMode.CUDA, "cuda"), (ExecMode.CPU, "cpu")):
        sim = make_sim(mode, 1024, per_world_rng=True)
        sim.step_n(3, random_actions=True, action_seed=321, step0=0)
        pol, opp = (FusedPolicy.from_agent(make_agent(s).to(dev)) for s in (8, 9))
        bufs = pol.rollout_buffers(sim, 16)
        pol.rollout(sim, 16, bufs, trainee=1, stochastic=True, seed=3, opponent=opp)
        outs.append(bufs)
    torch.cuda.synchronize()
    assert_same(outs[0], outs[1])


@pytest.mark.gpu
def test_gpu_selfplay_opponent_weights_are_the_opponents(native_lib):
    """An opponent with decisive logits changes the other agent's actions (the
    draws' uniforms are the same); the trainee's own weights as the opponent's
    still equal the per-step launches."""
    acts = [fused_vs_per_step(64, 4, 0, True, opp_seed=s, opp_gain=g)[1].action_tensor().to_torch()[:, 1].clone()
            for s, g in ((4, 1.0), (5, 300.0), (3, 1.0))]
    assert not torch.equal(acts[0], acts[1])
