// bb_policy_step_wide.h -- the tail of one PPO minibatch (bb_policy_step.h:
// clip_grad_norm_, Adam's step, the repack) for the policies of 184, 264, 344
// and 424 inputs.  The element math is bb_policy_step.h's, unchanged
// (adam_scalars, adam_element, step_powi); only the element order is wider:
// E = 32 IN + 1 876 parameter elements (7 764, 10 324, 12 884, 15 444), W1
// [32][IN] first, then b1 .. critic.b in the PG_* order, every offset behind W1
// the 128-wide one plus 32 (IN - 128); the four loss sums follow.  Shared by
// the host executor (bb_host.hip) and the gfx950 kernels
// (bb_policy_step_wide.hip).
#pragma once
#include "bb_policy_step.h"
#include "bb_policy_wide.h"

namespace bb {

BB_HD constexpr int psw_elems(int in_dim) { return pg_floats(in_dim) - 4; }              // E
BB_HD constexpr int psw_chunks(int in_dim) { return (pg_floats(in_dim) + PS_CHUNK - 1) / PS_CHUNK; }  // 122 .. 242
constexpr int PSW_CHUNKS_MAX = psw_chunks(PG_IN_MAX);
// workspace of the fused path behind ppo_grad_wide's: the unclipped gradient
// and the loss sums [E + 4] floats, then the chunk doubles, 16-byte aligned
BB_HD constexpr int64_t psw_ws_tail_bytes(int in_dim)
{
    return (((int64_t)pg_floats(in_dim) * 4 + (int64_t)psw_chunks(in_dim) * 8) + 15) / 16 * 16;
}

struct PolicyStepWideArgs {
    PolicyStepArgs s;          // param[0] / grad[0] / w.w1: [32][in_dim]; exp_avg / exp_avg_sq [E]; gsum [E + 4]; sq [chunks]
    int in_dim;
    // fused path, device only: pass 2's partials (s.partial / s.groups: pass 1's)
    const float *partial_w1;   // [groups_w1][32][in_dim]
    int groups_w1;
};

// Segment s (0..11) of the wide order.
BB_HD StepSeg step_seg_wide(const PolicyStepWideArgs &a, int s)
{
    StepSeg sg = step_seg(a.s, s);
    const int sh = POL_HID * (a.in_dim - POL_IN);
    if (s == 0) sg.len = sg.len + sh;
    else sg.e0 = sg.e0 + sh;
    return sg;
}

}  // namespace bb
