"""PPO update A/B at scripts/ppo.py's own shape: a 32 x 8 192-row buffer, 16
minibatches of 65 536 rows from torch.randperm per iteration, each minibatch
 (a) the torch path as update_policy writes it (get_minibatch, get_stats, the
     three losses, backward; scripts/ppo.py:190-213), or
 (b) FusedPolicy.ppo_grad (one gather + forward + loss + backward pass),
alternating in one process after warming both, device events around every
iteration.  Prints per-minibatch times with their spread and (b) against the
HBM floor of its gathered reads.

python tools/ppo_update_ab.py [--iters 10] [--trace DIR]
  --trace DIR: afterwards a kernel trace of (b) alone, `rocprofv3 --kernel-trace
  --stats` on a child process (--only-fused), under a time limit.
Exits non-zero on the first failure.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS, WORLDS, MINIBATCHES = 32, 8192, 4 * 4  # ppo.py:42's defaults: 4 epochs x 4 minibatches
CLIP, VF, ENT = 0.2, 1.0, 0.01
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--trace-timeout", type=int, default=240)
    a = ap.parse_args()
    import torch
    from madrona_basketball_amd.policy import BUCKETS, FusedPolicy, make_agent
    dev = torch.device("cuda")
    agent = make_agent(0).to(dev)
    pol = FusedPolicy.from_agent(agent)
    g = torch.Generator(device=dev).manual_seed(0)
    n = STEPS * WORLDS
    mb = n // 4
    buf = {"obs": torch.randn((STEPS, WORLDS, 128), device=dev, generator=g),
           "actions": torch.stack([torch.randint(0, nb, (STEPS, WORLDS), device=dev, generator=g) for nb in BUCKETS],
                                  -1).int(),
           "log_prob": -6.0 + 0.1 * torch.randn((STEPS, WORLDS), device=dev, generator=g),
           "value": torch.randn((STEPS, WORLDS), device=dev, generator=g),
           "adv": torch.randn((STEPS, WORLDS), device=dev, generator=g),
           "ret": torch.randn((STEPS, WORLDS), device=dev, generator=g)}
    flat = [buf["obs"].view(n, 128), buf["actions"].view(n, 6)] + [buf[k].view(n) for k in ("log_prob", "value", "adv", "ret")]
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
        pol.ppo_grad(*flat, idx=inds, clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)

    def iteration(fn):
        """One update_policy iteration's 16 minibatches; device ms."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(MINIBATCHES):
            if k % 4 == 0:
                b_inds = torch.randperm(n, device=dev)
            fn(b_inds[(k % 4) * mb:(k % 4 + 1) * mb])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    paths = {"fused": fused_minibatch} if a.only_fused else {"torch": torch_minibatch, "fused": fused_minibatch}
    for fn in paths.values():
        for _ in range(2):
            iteration(fn)
    ms = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, fn in paths.items():
            ms[k].append(iteration(fn))
    print(f"buffer {STEPS} x {WORLDS} rows, minibatch {mb}, {MINIBATCHES} minibatches per iteration, {a.iters} iterations"
          f" on {torch.cuda.get_device_name(0)}")
    for k, v in ms.items():
        us = [x * 1e3 / MINIBATCHES for x in v]
        print(f"{k:6s} per minibatch: median {statistics.median(us):9.1f} us  min {min(us):9.1f}  max {max(us):9.1f}  "
              f"(randperm included)")
    floor_us = mb * (512 + 24 + 16) / HBM_BYTES_PER_S * 1e6
    print(f"HBM floor of the gathered reads: {mb} x 552 B at {HBM_BYTES_PER_S / 1e12:.1f} TB/s = {floor_us:.1f} us")
    if "torch" in ms:
        print(f"torch / fused = {statistics.median(ms['torch']) / statistics.median(ms['fused']):.1f}")
    # the kernels alone: events around 20 back-to-back calls on one index set
    inds = torch.randperm(n, device=dev)[:mb]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fused_minibatch(inds)
    e1.record()
    e1.synchronize()
    print(f"fused call alone (20 back to back): {e0.elapsed_time(e1) * 1e3 / 20:.1f} us per minibatch")
    if a.trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace, "-o", "ppo_grad", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--only-fused", "--iters", "2"]
        subprocess.run(cmd, check=True, timeout=a.trace_timeout, cwd=ROOT)


if __name__ == "__main__":
    main()
