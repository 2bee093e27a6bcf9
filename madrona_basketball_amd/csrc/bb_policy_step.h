// bb_policy_step.h -- the tail of one PPO minibatch (scripts/ppo.py:214-215 and
// the repack the next minibatch needs): torch.nn.utils.clip_grad_norm_, then
// torch.optim.Adam's step (defaults: no weight decay, no amsgrad), then the new
// parameters into the packed weight image bb_policy_forward / k_ppo_grad read.
// Shared by the host executor (bb_host.hip) and the gfx950 kernels
// (bb_policy_step.hip).  Over the 5 972 parameter elements in PG_* order:
//
//   norm = sqrt(sum g^2) in double,  coef = min(1, max_norm / (norm + 1e-6))
//   g    = g coef                                   (also when coef is 1)
//   m    = m + (1 - beta1) (g - m)
//   v    = beta2 v + (1 - beta2) g g
//   den  = sqrt(v) / sqrt(1 - beta2^t) + eps        (eps outside the root, after the correction)
//   p    = p - (lr / (1 - beta1^t)) (m / den)
//
// t = 1, 2, ... is the step count after this step; the two corrections are
// computed once per call in double.  Every f32 operation below rounds on its
// own except where __builtin_fmaf says otherwise, so the fused and the
// standalone path give the same bits from the same gradient.
#pragma once
#include "bb_policy_grad.h"

namespace bb {

constexpr int PS_TENSORS = 12;        // agent.parameters(): w1 b1 ln1_w ln1_b w2 b2 ln2_w ln2_b actor.w actor.b critic.w critic.b
constexpr int PS_ELEMS = PG_LOSS;     // 5 972 parameter elements
constexpr int PS_CHUNK = 64;          // elements of one sum-of-squares partial
constexpr int PS_CHUNKS = (PG_FLOATS + PS_CHUNK - 1) / PS_CHUNK;  // 94: k_ppo_step's workgroups
// workspace of the fused path behind k_ppo_grad's partials: the unclipped
// gradient [PG_FLOATS], then PS_CHUNKS doubles
constexpr int64_t PS_WS_TAIL_BYTES = (int64_t)PG_FLOATS * 4 + (int64_t)PS_CHUNKS * 8;

struct AdamHyper {
    double lr, beta1, beta2, eps, max_norm;
};

// The scalars of one step, the same for every element.
struct AdamScalars {
    float coef;       // the clip factor
    float omb1;       // 1 - beta1
    float beta2;
    float omb2;       // 1 - beta2
    float bc2_sqrt;   // sqrt(1 - beta2^t)
    float eps;
    float step_size;  // lr / (1 - beta1^t)
    float norm;       // the gradient norm before clipping
};

// One segment of the PG_* order: a run of elements that lives in one
// parameter tensor (and one packed tensor).
struct StepSeg {
    float *param, *grad, *packed;  // at the segment's first element
    int e0, len;                   // PG_* offset and length
};

struct PolicyStepArgs {
    float *param[PS_TENSORS], *grad[PS_TENSORS];  // agent.parameters() order
    PolicyWeights w;                              // the packed image (written)
    float *exp_avg, *exp_avg_sq;                  // [5972], PG_* order
    int64_t *step;                                // [1]
    int32_t *ticket;                              // [1], device only; 0 between calls
    AdamHyper h;
    float *out;                                   // standalone: norm, coef; fused: loss4, norm, coef
    // fused path, device only
    const float *partial;                         // k_ppo_grad's [groups][PG_FLOATS]
    int groups;
    float *gsum;                                  // [PG_FLOATS] the unclipped gradient and loss sums
    double *sq;                                   // [PS_CHUNKS] sums of squares
};

// Segment s (0..11) of the PG_* order.  Static s: folds to constants.
BB_HD StepSeg step_seg(const PolicyStepArgs &a, int s)
{
    constexpr int AW = POL_LOGITS * POL_HID;  // actor.weight's 608 floats
    float *const hw = const_cast<float *>(a.w.head_w), *const hb = const_cast<float *>(a.w.head_b);
    switch (s) {
    case 0: return {a.param[0], a.grad[0], const_cast<float *>(a.w.w1), PG_W1, PG_B1 - PG_W1};
    case 1: return {a.param[1], a.grad[1], const_cast<float *>(a.w.b1), PG_B1, POL_HID};
    case 2: return {a.param[2], a.grad[2], const_cast<float *>(a.w.ln1_w), PG_LN1W, POL_HID};
    case 3: return {a.param[3], a.grad[3], const_cast<float *>(a.w.ln1_b), PG_LN1B, POL_HID};
    case 4: return {a.param[4], a.grad[4], const_cast<float *>(a.w.w2), PG_W2, PG_B2 - PG_W2};
    case 5: return {a.param[5], a.grad[5], const_cast<float *>(a.w.b2), PG_B2, POL_HID};
    case 6: return {a.param[6], a.grad[6], const_cast<float *>(a.w.ln2_w), PG_LN2W, POL_HID};
    case 7: return {a.param[7], a.grad[7], const_cast<float *>(a.w.ln2_b), PG_LN2B, POL_HID};
    case 8: return {a.param[8], a.grad[8], hw, PG_HW, AW};                      // actor.weight: head rows 0-18
    case 9: return {a.param[10], a.grad[10], hw + AW, PG_HW + AW, POL_HID};     // critic.weight: head row 19
    case 10: return {a.param[9], a.grad[9], hb, PG_HB, POL_LOGITS};             // actor.bias
    default: return {a.param[11], a.grad[11], hb + POL_LOGITS, PG_HB + POL_LOGITS, 1};  // critic.bias
    }
}

BB_HD double step_powi(double b, int64_t t)
{
    double r = 1.0;
    for (; t > 0; t >>= 1) {
        if (t & 1) r = r * b;
        b = b * b;
    }
    return r;
}

// The step's scalars from the sum of squares and the step count t >= 1.
BB_HD AdamScalars adam_scalars(const AdamHyper &h, double sumsq, int64_t t)
{
    const double norm = bbm::sqrt_d(sumsq);
    const double c = h.max_norm / (norm + 1e-6);
    AdamScalars s;
    s.coef = (float)(c < 1.0 ? c : 1.0);
    s.omb1 = (float)(1.0 - h.beta1);
    s.beta2 = (float)h.beta2;
    s.omb2 = (float)(1.0 - h.beta2);
    s.bc2_sqrt = (float)bbm::sqrt_d(1.0 - step_powi(h.beta2, t));
    s.eps = (float)h.eps;
    s.step_size = (float)(h.lr / (1.0 - step_powi(h.beta1, t)));
    s.norm = (float)norm;
    return s;
}

// One element: the raw gradient g in, the clipped gradient out; m, v, p updated.
BB_HD float adam_element(const AdamScalars &s, float g, float *m, float *v, float *p)
{
#pragma clang fp contract(off)
    const float gc = g * s.coef;
    const float m1 = __builtin_fmaf(s.omb1, gc - *m, *m);
    const float v1 = __builtin_fmaf(s.omb2 * gc, gc, s.beta2 * *v);
    const float den = bbm::sqrtf_(v1) / s.bc2_sqrt + s.eps;
    *m = m1;
    *v = v1;
    *p = *p - s.step_size * (m1 / den);
    return gc;
}

}  // namespace bb
