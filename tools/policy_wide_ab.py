"""Policy inference A/B at the observation widths of 4 and 10 agents: every
agent's rows of 65 536 x 4 (262 144 rows x 184) and 8 192 x 10 (81 920 rows x
424), argmax and sampled, each call
 (a) the torch path, fp32 Agent.forward as scripts/agent.py:140-154 writes it
     (obs_norm, backbone, heads, a Categorical per bucket: best() or sample(),
     log_prob; scripts/action.py), or
 (b) FusedPolicy.__call__ (bb_policy_forward_wide, one launch),
alternating in one process after warming both, device events around every
window of 50 back-to-back calls.  Prints the median and the spread per path
and (b) against the HBM floor rows x (4 IN + 32) B at 8 TB/s.

python tools/policy_wide_ab.py [--repeats 20]
Exits non-zero on the first failure.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((65536, 4, 184), (8192, 10, 424))  # worlds, agents, bb_obs_width(agents)
HBM_BYTES_PER_S = 8.0e12  # MI355X peak
CALLS = 50  # per timed window


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    if a.repeats < 10:
        ap.error("at least 10 repeats")
    import torch
    from madrona_basketball_amd.policy import BUCKETS, FusedPolicy, make_agent
    dev = torch.device("cuda")
    print(f"{a.repeats} alternating windows of {CALLS} calls on {torch.cuda.get_device_name(0)}; "
          "us per call: median (min .. max)")
    for worlds, n, width in SHAPES:
        rows = worlds * n
        agent = make_agent(0, input_dim=width).to(dev)
        pol = FusedPolicy.from_agent(agent)
        obs = torch.randn((rows, width), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        mean, inv = pol._tensors["obs_mean"], pol._tensors["obs_inv"]

        @torch.no_grad()
        def torch_call(stochastic):
            x = agent.backbone(torch.clamp((obs - mean) * inv, -5.0, 5.0))
            logits, value = agent.actor(x), agent.critic(x).squeeze(-1)
            acts, lps, off = [], [], 0
            for nb in BUCKETS:
                d = torch.distributions.Categorical(logits=logits[:, off:off + nb])
                act = d.sample() if stochastic else d.probs.argmax(dim=-1)
                acts.append(act)
                lps.append(d.log_prob(act))
                off += nb
            return torch.stack(acts, 1), torch.stack(lps, 1).sum(-1), value

        def fused_call(stochastic):
            return pol(obs, stochastic=stochastic, seed=1, step=2)

        def timed(fn, stochastic):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn(stochastic)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / CALLS

        floor_us = rows * (4 * width + 32) / HBM_BYTES_PER_S * 1e6
        for stochastic in (False, True):
            paths = {"torch": torch_call, "fused": fused_call}
            for fn in paths.values():
                for _ in range(3):
                    timed(fn, stochastic)
            us = {k: [] for k in paths}
            for _ in range(a.repeats):
                for k, fn in paths.items():
                    us[k].append(timed(fn, stochastic))
            med = {k: statistics.median(v) for k, v in us.items()}
            print(f"{worlds} x {n} = {rows} rows x {width}, {'sampled' if stochastic else 'argmax'}:")
            for k, v in us.items():
                print(f"  {k:5s} {med[k]:9.1f} ({min(v):.1f} .. {max(v):.1f})")
            print(f"  torch / fused = {med['torch'] / med['fused']:.1f}; HBM floor {floor_us:.1f} us, "
                  f"floor / fused = {floor_us / med['fused']:.2f}")
            if min(us["torch"]) <= max(us["fused"]):
                print("  the two paths' ranges overlap")


if __name__ == "__main__":
    main()
