"""Self-play in the fused PPO step (k_rollout_ppo's opponent form: bb_rollout_policy
with a frozen opponent above the fused rollout's bound, in one launch) == the
per-step launches and the host executor, every record and every column, bit
for bit.  The path is forced at small world counts through the overrides."""
import pytest
import torch

from madrona_basketball_amd import ExecMode, _lib
from madrona_basketball_amd.policy import FusedPolicy, make_agent
from tests.helpers import make_sim
from tests.test_policy_rollout import assert_same

FUSED_STEP, PER_STEP = 2, 3  # BB_PPO_PATH_*
FORCE = dict(ppo_fused_max_worlds=0, ppo_selfplay_step_min_worlds=1)


@pytest.mark.gpu
def test_gpu_selfplay_step_path(native_lib):
    sim = make_sim(ExecMode.CUDA, 64)
    with _lib.diag(**FORCE):
        assert native_lib.bb_rollout_policy_path(sim._h, 1, 0) == FUSED_STEP
        assert native_lib.bb_rollout_policy_path(sim._h, 1, _lib.ROLLOUT_PER_STEP) == PER_STEP
        with _lib.diag(ppo_step_loop=0):  # k_step_ppo has no opponent form
            assert native_lib.bb_rollout_policy_path(sim._h, 1, 0) == PER_STEP


def step_vs_per_step(W, n, trainee, stochastic, opp_seed=4, opp_gain=1.0):
    sims = [make_sim(ExecMode.CUDA, W, per_world_rng=True) for _ in range(2)]
    for s in sims:
        s.step_n(9, random_actions=True, action_seed=321, step0=0)
    pol = FusedPolicy.from_agent(make_agent(3).cuda())
    opp_agent = make_agent(opp_seed)
    opp_agent.actor.weight.data.mul_(opp_gain)  # (make_agent's heads have gain 0.01: logits near 0)
    opp = FusedPolicy.from_agent(opp_agent.cuda())
    bufs = [pol.rollout_buffers(s, n) for s in sims]
    with _lib.diag(**FORCE):
        assert _lib.load().bb_rollout_policy_path(sims[0]._h, 1, 0) == FUSED_STEP
        for s, b, per_step in zip(sims, bufs, (False, True)):
            pol.rollout(s, n, b, trainee=trainee, stochastic=stochastic, seed=11, step0=5, opponent=opp,
                        per_step=per_step)
    torch.cuda.synchronize()
    assert_same(bufs[0], bufs[1])
    for name in sims[0]._views:
        assert torch.equal(sims[0]._views[name], sims[1]._views[name]), name
    return bufs[0], sims[0]


@pytest.mark.gpu
@pytest.mark.parametrize("W,n,trainee,stochastic", [
    (31, 4, 1, True),       # one partial wave
    (33, 1, 0, True),       # one wave plus one world; the step-0 pass with the opponent, then the value pass only
    (64, 3, 0, False),      # an argmax trainee beside the sampling opponent
    (1000, 20, 1, True),    # a partial last workgroup
    (40000, 5, 0, True),    # more workgroups than CUs
    (1000, 640, 0, True),   # across the 620-step clock expiry and the in-launch reset
])
def test_gpu_selfplay_step_equals_per_step_launches(native_lib, W, n, trainee, stochastic):
    bufs, _ = step_vs_per_step(W, n, trainee, stochastic)
    if n > 620:
        assert (bufs["done"] == 1).any(dim=0).all()  # every world was reset inside the launch


@pytest.mark.gpu
def test_gpu_selfplay_step_equals_host_executor(native_lib):
    outs = []
    for mode, dev in ((ExecMode.CUDA, "cuda"), (ExecMode.CPU, "cpu")):
        sim = make_sim(mode, 1024, per_world_rng=True)
        sim.step_n(3, random_actions=True, action_seed=321, step0=0)
        pol, opp = (FusedPolicy.from_agent(make_agent(s).to(dev)) for s in (8, 9))
        bufs = pol.rollout_buffers(sim, 16)
        with _lib.diag(**FORCE):
            assert mode == ExecMode.CPU or native_lib.bb_rollout_policy_path(sim._h, 1, 0) == FUSED_STEP
            pol.rollout(sim, 16, bufs, trainee=1, stochastic=True, seed=3, opponent=opp)
        outs.append(bufs)
    torch.cuda.synchronize()
    assert_same(outs[0], outs[1])


@pytest.mark.gpu
def test_gpu_selfplay_step_opponent_weights_are_the_opponents(native_lib):
    """An opponent with decisive logits changes the other agent's actions (the
    draws' uniforms are the same); both runs equal their per-step twins."""
    acts = [step_vs_per_step(64, 4, 0, True, opp_seed=s, opp_gain=g)[1].action_tensor().to_torch()[:, 1].clone()
            for s, g in ((4, 1.0), (5, 300.0))]
    assert not torch.equal(acts[0], acts[1])
