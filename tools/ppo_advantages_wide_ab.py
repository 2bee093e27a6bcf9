"""compute_advantages A/B at the wide observation widths (184 to 424 columns),
a 32 x 8 192 rollout buffer, per iteration
 (a) the torch path as the reference writes it (scripts/ppo.py:144-177 over
     RunningMeanStd, scripts/agent.py:28-50) at that width, or
 (b) FusedPolicy.compute_advantages (k_adv_scan_wide, k_adv_finish_wide,
     k_adv_norm),
alternating in one process after warming both, device events around every call.
Prints median / min / max per call and (b) against the HBM floor of its bytes.

python tools/ppo_advantages_wide_ab.py [--width 184] [--iters 20] [--trace DIR]
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

STEPS, WORLDS = 32, 8192
GAMMA, LAM = 0.998, 0.95
HBM_BYTES_PER_S = 8.0e12  # MI355X peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=184, choices=(184, 264, 344, 424))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-fused", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--trace-timeout", type=int, default=240)
    a = ap.parse_args()
    import torch
    from madrona_basketball_amd.policy import FusedPolicy, RunningStats, make_agent
    dev, width = torch.device("cuda"), a.width
    pol = FusedPolicy.from_agent(make_agent(0, input_dim=width).to(dev))
    g = torch.Generator(device=dev).manual_seed(0)
    shape = (STEPS, WORLDS)
    buf = {"obs": torch.randn((*shape, width), device=dev, generator=g) * 3 + 1,
           "value": torch.randn(shape, device=dev, generator=g),
           "reward": torch.randn(shape, device=dev, generator=g) * 0.1,
           "done": (torch.rand(shape, device=dev, generator=g) < 0.01).float(),
           "next_value": torch.randn((WORLDS,), device=dev, generator=g)}
    adv, ret = torch.empty(shape, device=dev), torch.empty(shape, device=dev)
    norms = {k: (RunningStats(1, dev), RunningStats(width, dev)) for k in ("torch", "fused")}

    def forward(st, x, unnorm=False):  # agent.py:28-38 with clamp 5
        mean, var = st.mean.to(torch.float32), st.var.to(torch.float32) + 1e-5
        if unnorm:
            return mean + torch.sqrt(var) * torch.clamp(x, min=-5.0, max=5.0)
        return torch.clamp((x - mean) * torch.rsqrt(var), min=-5.0, max=5.0)

    def update(st, x):  # agent.py:41-50
        var, mean = torch.var_mean(x, dim=0, unbiased=True)
        count = x.size(0)
        count_ = count + st.count
        delta = mean - st.mean
        m = st.var * st.count + var * count + delta ** 2 * st.count * count / count_
        st.mean.copy_(st.mean + delta * count / count_)
        st.var.copy_(m / count_)
        st.count.copy_(count_)

    @torch.no_grad()
    def torch_path():  # ppo.py:144-177
        vn, on = norms["torch"]
        not_dones = 1 - buf["done"]  # the reference's buffer stores not_dones; one extra pass here
        values, next_value = forward(vn, buf["value"], True), forward(vn, buf["next_value"], True)
        adv[:] = 0.0
        last = 0.0
        for t in reversed(range(STEPS)):
            if t == STEPS - 1:
                nnt, nxt = not_dones[t], next_value
            else:
                nnt, nxt = not_dones[t + 1], values[t + 1]
            delta = buf["reward"][t] + GAMMA * nxt * nnt - values[t]
            adv[t] = last = delta + GAMMA * LAM * nnt * last
        ret[:] = adv + values
        update(on, buf["obs"].view(-1, width))
        update(vn, values.view(-1, 1))
        update(vn, ret.view(-1, 1))
        mu, sigma = adv.mean(), adv.std()
        adv[:] = (adv - mu) / (sigma + 1e-8)
        values[:] = forward(vn, values)
        ret[:] = forward(vn, ret)

    def fused_path():
        vn, on = norms["fused"]
        pol.compute_advantages(buf, adv, ret, vn, on, GAMMA, LAM)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    paths = {"fused": fused_path} if a.only_fused else {"torch": torch_path, "fused": fused_path}
    for fn in paths.values():
        for _ in range(3):
            timed(fn)
    us = {k: [] for k in paths}
    for _ in range(a.iters):
        for k, fn in paths.items():
            us[k].append(timed(fn))
    print(f"width {width}, buffer {STEPS} x {WORLDS} rows, {a.iters} alternating calls on {torch.cuda.get_device_name(0)}")
    for k, v in us.items():
        print(f"{k:6s} per call: median {statistics.median(v):9.1f} us  min {min(v):9.1f}  max {max(v):9.1f}")
    rows = STEPS * WORLDS
    # obs once, the three [K, W] inputs once, advantages / returns written, read and written again
    nbytes = rows * (4 * width + 3 * 4 + 2 * 3 * 4) + WORLDS * 4
    floor_us = nbytes / HBM_BYTES_PER_S * 1e6
    print(f"HBM floor: {nbytes} B at {HBM_BYTES_PER_S / 1e12:.1f} TB/s = {floor_us:.1f} us; "
          f"fused / floor = {statistics.median(us['fused']) / floor_us:.1f}")
    if "torch" in us:
        print(f"torch / fused = {statistics.median(us['torch']) / statistics.median(us['fused']):.1f}")
    if a.trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", a.trace, "-o", f"ppo_advantages_wide_{width}",
               "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--only-fused", "--iters", "20",
               "--width", str(width)]
        subprocess.run(cmd, check=True, timeout=a.trace_timeout, cwd=ROOT)


if __name__ == "__main__":
    main()
