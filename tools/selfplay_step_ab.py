"""Self-play PPO rollout above the fused rollout's bound, A/B: bb_rollout_policy
with a frozen opponent, K = 32, all records, as
 (a) the per-step launches (per_step=True: a k_policy launch per acting agent
     and a k_step launch per step),
 (b) the fused self-play step (k_rollout_ppo's opponent form, one launch) at 4
     waves per workgroup, and
 (c) the same at 6 waves per workgroup,
alternating in one process after warming all three, device events around every
rollout.  The workgroup size is a compile-time constant of the library
(BB_PPO_SELFPLAY_WPG), so (b) and (c) are two builds of it loaded side by side:
the product's and a variant,

    python -m madrona_basketball_amd.build --variant selfplay_wpg6 -D BB_PPO_SELFPLAY_WPG=6   (or =4)

python tools/selfplay_step_ab.py [--worlds 24576,32768,65536] [--reps 3] [--rollouts 20]
                                 [--variant selfplay_wpg6]
Prints per leg and world count the per-step microseconds of every repeat, their
median and their spread (max - min).  Exits non-zero on the first failure.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="24576,32768,65536")
    ap.add_argument("--reps", type=int, default=3, help="interleaved repeats per leg")
    ap.add_argument("--rollouts", type=int, default=20, help="timed rollouts per repeat")
    ap.add_argument("--variant", default="selfplay_wpg6", help="the other workgroup size's build under _variants/")
    a = ap.parse_args()
    import torch
    import madrona_basketball_amd as mba
    from madrona_basketball_amd import _lib
    from madrona_basketball_amd.policy import FusedPolicy, make_agent

    # the two builds, each with its own simulators and overrides; `use` makes
    # one of them the library the package calls
    libs = {"product": _lib.load()}
    _lib._lib = None
    os.environ["MADRONA_BB_LIB"] = os.path.join(ROOT, "madrona_basketball_amd", "_variants", a.variant,
                                                "libmadrona_basketball_amd.so")
    libs["variant"] = _lib.load()
    del os.environ["MADRONA_BB_LIB"]

    def use(which):
        _lib._lib = libs[which]

    product_wpg = 6 if a.variant.endswith("4") else 4
    legs = [("per-step launches", "product", True), (f"fused step WPG {product_wpg}", "product", False),
            (f"fused step WPG {10 - product_wpg}", "variant", False)]
    pol = FusedPolicy.from_agent(make_agent(0).cuda())
    opp = FusedPolicy.from_agent(make_agent(1).cuda())
    print(f"self-play bb_rollout_policy, K = {K}, all records, {a.reps} interleaved repeats of {a.rollouts} rollouts"
          f" on {torch.cuda.get_device_name(0)}; us per step")
    for W in (int(w) for w in a.worlds.split(",")):
        sims, bufs = {}, {}
        for which in libs:
            use(which)
            _lib.diag_set("ppo_selfplay_step_min_worlds", 16385)
            sims[which] = mba.SimpleGridworldSimulator(32, 17, 15.7575, 8.382, 39600, mba.ExecMode.CUDA, W, 0,
                                                       per_world_rng=True)
            bufs[which] = pol.rollout_buffers(sims[which], K)

        def leg(which, per_step, rollouts, step0):
            use(which)
            want = 3 if per_step else 2  # BB_PPO_PATH_PER_STEP / FUSED_STEP
            got = libs[which].bb_rollout_policy_path(sims[which]._h, 1, _lib.ROLLOUT_PER_STEP if per_step else 0)
            assert got == want, (which, per_step, got)
            ms = sum(pol.rollout(sims[which], K, bufs[which], seed=1, step0=step0 + i * K, opponent=opp,
                                 per_step=per_step, time_kernels=True) for i in range(rollouts))
            return ms * 1e3 / (rollouts * K)

        for _, which, per_step in legs:
            leg(which, per_step, 2, 0)
        us = {name: [] for name, _, _ in legs}
        for r in range(a.reps):
            for name, which, per_step in legs:
                us[name].append(leg(which, per_step, a.rollouts, (r + 1) * a.rollouts * K))
        for name, v in us.items():
            print(f"{W:7d} worlds  {name:20s} " + " ".join(f"{x:7.2f}" for x in v)
                  + f"   median {statistics.median(v):7.2f}  spread {max(v) - min(v):5.2f}", flush=True)
        torch.cuda.synchronize()
        for which in libs:  # each simulator destroyed by the build that created it
            use(which)
            del sims[which]
    use("product")


if __name__ == "__main__":
    main()
