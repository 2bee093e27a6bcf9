"""PPO update A/B at the wide observation widths (184 to 424 inputs), at
scripts/ppo.py's shape: a 32 x 8 192-row buffer, 4 epochs x 4 minibatches of
65 536 rows from torch.randperm per iteration, as
 (a) FusedPolicy.ppo_grad_wide, then torch.nn.utils.clip_grad_norm_, then
     torch.optim.Adam.step(), then FusedPolicy.refresh() per minibatch (what a
     user of these widths ran before ppo_update served them), or
 (b) FusedPolicy.ppo_update (k_ppo_grad_wide, k_ppo_dw1, k_ppo_step_wide,
     k_adam_step_wide per minibatch),
alternating in one process after warming both, device events around every
16-minibatch iteration.

python tools/ppo_step_wide_ab.py [--width 184] [--iters 10] [--trace DIR]
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

STEPS, WORLDS, EPOCHS, MINIBATCHES = 32, 8192, 4, 4  # ppo.py:42-48's defaults
CLIP, VF, ENT, LR, MAX_NORM = 0.2, 1.0, 0.01, 3e-4, 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=184, choices=(184, 264, 344, 424))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--trace-timeout", type=int, default=240)
    a = ap.parse_args()
    import torch
    from madrona_basketball_amd.policy import BUCKETS, AdamState, FusedPolicy, make_agent
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    n = STEPS * WORLDS
    mb = n // MINIBATCHES
    flat = [torch.randn((n, a.width), device=dev, generator=g),
            torch.stack([torch.randint(0, nb, (n,), device=dev, generator=g) for nb in BUCKETS], -1).int(),
            -6.0 + 0.1 * torch.randn((n,), device=dev, generator=g)] + [torch.randn((n,), device=dev, generator=g)
                                                                         for _ in range(3)]
    coefs = dict(clip_coef=CLIP, vf_coef=VF, ent_coef=ENT)

    def torch_tail():
        agent = make_agent(0, input_dim=a.width).to(dev)
        pol, opt = FusedPolicy.from_agent(agent), torch.optim.Adam(agent.parameters(), lr=LR, eps=1e-8)

        def run():
            for _ in range(EPOCHS):
                b_inds = torch.randperm(n, device=dev)
                for start in range(0, n, mb):
                    pol.ppo_grad_wide(*flat, idx=b_inds[start:start + mb], **coefs)
                    torch.nn.utils.clip_grad_norm_(agent.parameters(), MAX_NORM)
                    opt.step()
                    pol.refresh()
        return run

    def fused():
        pol = FusedPolicy.from_agent(make_agent(0, input_dim=a.width).to(dev))
        state = AdamState(dev, in_dim=a.width)
        return lambda: pol.ppo_update(*flat, state, update_epochs=EPOCHS, num_minibatches=MINIBATCHES, lr=LR,
                                      max_grad_norm=MAX_NORM, **coefs)

    def iteration(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    paths = {"ppo_update": fused()}
    if not a.only_fused:
        paths = {"torch tail": torch_tail(), **paths}
    for fn in paths.values():
        for _ in range(2):
            iteration(fn)
    ms = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, fn in paths.items():
            ms[k].append(iteration(fn))
    steps = EPOCHS * MINIBATCHES
    print(f"width {a.width}, buffer {STEPS} x {WORLDS} rows, minibatch {mb}, {steps} minibatches per iteration, "
          f"{a.iters} iterations on {torch.cuda.get_device_name(0)}")
    for k, v in ms.items():
        us = [x * 1e3 / steps for x in v]
        print(f"{k:10s} per minibatch: median {statistics.median(us):9.1f} us  min {min(us):9.1f}  max {max(us):9.1f}  "
              f"(randperm included)")
    if "torch tail" in ms:
        print(f"torch tail / ppo_update = {statistics.median(ms['torch tail']) / statistics.median(ms['ppo_update']):.2f}")
    if a.trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace, "-o", f"ppo_step_wide_{a.width}",
               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--only-fused", "--iters", "2",
               "--width", str(a.width)]
        subprocess.run(cmd, check=True, timeout=a.trace_timeout, cwd=ROOT)


if __name__ == "__main__":
    main()
