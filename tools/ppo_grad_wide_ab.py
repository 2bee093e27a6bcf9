"""PPO loss + gradient A/B at the wide observation rows: 65 536-row minibatches
of torch.randperm out of a 262 144 x 184 buffer (2v2) and 40 960-row ones out
of an 81 920 x 424 buffer (5v5, the buffer split in two) -- tools/policy_wide_ab.py's
shapes -- each minibatch
 (a) the torch path as update_policy writes it (get_minibatch, get_stats, the
     three losses, backward; scripts/ppo.py:190-213), the only path these widths
     had, or
 (b) FusedPolicy.ppo_grad_wide (two gathered passes and a reduce),
alternating in one process after warming both, device events around every
iteration of 8 minibatches.  Prints per-minibatch median / min / max and (b)
against the HBM floor of its two gathered reads.

python tools/ppo_grad_wide_ab.py [--iters 10]
Exits non-zero on the first failure.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((184, 262144, 65536), (424, 81920, 40960))  # width, buffer rows, minibatch rows
MINIBATCHES = 8
CLIP, VF, ENT = 0.2, 1.0, 0.01
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    import torch
    from madrona_basketball_amd.policy import BUCKETS, FusedPolicy, make_agent
    dev = torch.device("cuda")
    print(f"{MINIBATCHES} minibatches per iteration, {a.iters} iterations on {torch.cuda.get_device_name(0)}")
    for width, n, mb in SHAPES:
        agent = make_agent(0, input_dim=width).to(dev)
        pol = FusedPolicy.from_agent(agent)
        g = torch.Generator(device=dev).manual_seed(0)
        flat = [torch.randn((n, width), device=dev, generator=g),
                torch.stack([torch.randint(0, nb, (n,), device=dev, generator=g) for nb in BUCKETS], -1).int(),
                -6.0 + 0.1 * torch.randn((n,), device=dev, generator=g)]
        flat += [torch.randn((n,), device=dev, generator=g) for _ in range(3)]  # value, advantages, returns
        mean, inv = pol._tensors["obs_mean"], pol._tensors["obs_inv"]

        def torch_minibatch(inds):
            o, act, lp, v, adv, ret = (t[inds] for t in flat)  # buffers.py:25-33
            x = agent.backbone(torch.clamp((o - mean) * inv, -5.0, 5.0))  # agent.py:172-178
            logits, v_ = agent.actor(x), agent.critic(x).squeeze(-1)
            lps, es, off = [], [], 0
            for b, nb in enumerate(BUCKETS):  # action.py:35-44
                d = torch.distributions.Categorical(logits=logits[:, off:off + nb])
                lps.append(d.log_prob(act[:, b].long()))
                es.append(d.entropy())
                off += nb
            lp_, e = torch.stack(lps, 1).sum(-1), torch.stack(es, 1).sum(-1)
            ratio = torch.exp(lp_ - lp)  # ppo.py:195-210
            pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
            v_clip = v + (v_ - v).clamp(-CLIP, CLIP)
            c = 0.5 * torch.max((v_ - ret) ** 2, (v_clip - ret) ** 2).mean() * VF
            loss = pg + c - e.mean() * ENT
            for p in agent.parameters():
                p.grad = None
            loss.backward()

        def fused_minibatch(inds):
            pol.ppo_grad_wide(*flat, idx=inds, clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)

        per_perm = n // mb

        def iteration(fn):
            """MINIBATCHES minibatches, a new permutation whenever one is used up; device ms."""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(MINIBATCHES):
                if k % per_perm == 0:
                    b_inds = torch.randperm(n, device=dev)
                fn(b_inds[(k % per_perm) * mb:(k % per_perm + 1) * mb])
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        paths = {"torch": torch_minibatch, "fused": fused_minibatch}
        for fn in paths.values():
            for _ in range(2):
                iteration(fn)
        ms = {k: [] for k in paths}
        for _ in range(a.iters):
            for k, fn in paths.items():
                ms[k].append(iteration(fn))
        print(f"buffer {n} x {width}, minibatch {mb}")
        for k, v in ms.items():
            us = [x * 1e3 / MINIBATCHES for x in v]
            print(f"  {k:6s} per minibatch: median {statistics.median(us):9.1f} us  min {min(us):9.1f}  max {max(us):9.1f}"
                  f"  (randperm included)")
        floor_us = mb * (2 * 4 * width + 40) / HBM_BYTES_PER_S * 1e6
        print(f"  HBM floor of the two gathered reads: {mb} x {2 * 4 * width + 40} B at "
              f"{HBM_BYTES_PER_S / 1e12:.1f} TB/s = {floor_us:.1f} us")
        print(f"  torch / fused = {statistics.median(ms['torch']) / statistics.median(ms['fused']):.1f}")
        # the kernels alone: events around 20 back-to-back calls on one index set
        inds = torch.randperm(n, device=dev)[:mb]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fused_minibatch(inds)
        e1.record()
        e1.synchronize()
        print(f"  fused call alone (20 back to back): {e0.elapsed_time(e1) * 1e3 / 20:.1f} us per minibatch")


if __name__ == "__main__":
    main()
