/*
 * madrona_basketball_amd.h -- C ABI of the MI355X-native batched basketball
 * simulator (the drop-in boundary for the reference's step path).
 *
 * Each entry point replaces one piece of the reference's Manager / nanobind
 * surface (davidj24/madrona_basketball):
 *
 *   bb_create / bb_create_with_buffers
 *       <- Manager::Manager(Config, GridState)        src/mgr.cpp:236-239
 *          + the binding's ctor                        src/bindings.cpp:18-61
 *   bb_destroy          <- Manager::~Manager           src/mgr.cpp:241
 *   bb_step             <- Manager::step               src/mgr.cpp:243-246
 *   bb_step_n           <- n x Manager::step (+ optional on-device random
 *                          actions, the bench workload of scripts/run.py:6-19)
 *   bb_step_n_staged    <- n x (actions[:] = a_k; Manager::step), the
 *                          scripts/run.py:10-15 loop with a_k staged in HBM
 *   bb_fill_random_actions <- (new) stages a_k for bb_step_n_staged
 *   bb_rollout          <- n x (actions[:] = a_k; Manager::step; copy of
 *                          observations/rewards/dones), the rollout loop of
 *                          scripts/ppo.py:61-141 with a_k staged in HBM
 *   bb_record           <- the per-step trajectory logging of scripts/ppo.py:93-106
 *                          and scripts/infer.py:116-129 (ten .cpu() copies per
 *                          step), as one device-side copy into a ring
 *   bb_policy_forward   <- Agent.forward of scripts/agent.py:140-154 (32 channels,
 *                          2 layers, env.py:107) + the action write of
 *                          scripts/env.py:147, fused on the device
 *   bb_policy_forward_wide <- the same for Agent(envs.get_input_dim(), ...) at the
 *                          184 / 264 / 344 / 424-float rows of 4 to 10 agents
 *   bb_rollout_policy   <- rollout() of scripts/ppo.py:61-141: n x (agent(obs);
 *                          env.step; buffer stores) + agent.evaluate(obs_)
 *   bb_set_action       <- Manager::setAction          src/mgr.cpp:270-293
 *   bb_trigger_reset    <- Manager::triggerReset       src/mgr.cpp:297-311
 *   bb_export           <- Manager::*Tensor() getters  src/mgr.cpp:317-445
 *                          (exportTensor, src/mgr.cpp:74-80, 121-126)
 *   bb_buffer_bytes     <- (new) sizes for caller-owned storage
 *   bb_last_error       <- (new) the reference aborts via FATAL/REQ_CUDA
 *                          (src/mgr.cpp:191,198) or printf (:289-292);
 *                          this ABI returns status codes instead.
 *
 * Plain C types only.  All device pointers are HIP device pointers on the
 * simulator's gpu_id; `stream` is a hipStream_t passed as void* (NULL = the
 * default stream).  No function aborts; every function returns BB_OK or a
 * negative error code and records a message for bb_last_error().
 */
#ifndef MADRONA_BASKETBALL_AMD_H
#define MADRONA_BASKETBALL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BB_ABI_VERSION 1

/* status codes */
#define BB_OK 0
#define BB_ERR_INVALID_ARG (-1)
#define BB_ERR_UNSUPPORTED (-2)
#define BB_ERR_HIP (-3)
#define BB_ERR_OOM (-4)

/* madrona::ExecMode (madrona_basketball.madrona.ExecMode) */
#define BB_EXEC_CPU 0
#define BB_EXEC_CUDA 1   /* the HIP/gfx950 path; named as in the reference */

/* dtypes reported by bb_export (madrona::py::TensorElementType subset) */
#define BB_DTYPE_INT32 0
#define BB_DTYPE_FLOAT32 1

/* config flags */
#define BB_FLAG_PER_WORLD_RNG 0x1u /* key each world's RNG by its global index
                                      (reference: every world shares key
                                      split_i(initKey(0),0,0), src/sim.cpp:89) */
#define BB_FLAG_NO_TAG_MASK   0x2u /* drop the tag override of game.cpp:526-528 */
#define BB_FLAG_FULL_GAME     0x4u /* isOneOnOne = 0 (constants.hpp:27 = 0) */

/* Export ids: exactly src/types.hpp:10-42, then build-internal state. */
#define BB_EXPORT_RESET 0
#define BB_EXPORT_GAME_STATE 1
#define BB_EXPORT_ACTION 2
#define BB_EXPORT_ACTION_MASK 3
#define BB_EXPORT_AGENT_POS 4
#define BB_EXPORT_OBSERVATIONS 5
#define BB_EXPORT_REWARD 6
#define BB_EXPORT_DONE 7
#define BB_EXPORT_AGENT_ENTITY_ID 8
#define BB_EXPORT_AGENT_POSSESSION 9
#define BB_EXPORT_ORIENTATION 10
#define BB_EXPORT_TEAM 11
#define BB_EXPORT_AGENT_STATS 12
#define BB_EXPORT_BALL_POS 13
#define BB_EXPORT_BALL_PHYSICS 14
#define BB_EXPORT_BALL_ENTITY_ID 15
#define BB_EXPORT_BALL_GRABBED 16
#define BB_EXPORT_BALL_VELOCITY 17
#define BB_EXPORT_HOOP_POS 18
#define BB_NUM_REFERENCE_EXPORTS 19
#define BB_INTERNAL_AGENT_VELOCITY 32
#define BB_INTERNAL_GRAB_COOLDOWN 33
#define BB_INTERNAL_CUR_STEP 34
#define BB_INTERNAL_INBOUNDING 35
#define BB_INTERNAL_ATTRIBUTES 36
#define BB_INTERNAL_WORLD_CLOCK 37
#define BB_INTERNAL_RNG_COUNTER 38
#define BB_INTERNAL_FIRST 32
#define BB_INTERNAL_LAST 38

typedef struct bb_sim bb_sim;

typedef struct bb_config {
    int64_t discrete_x;          /* grid cells, cellsPerMeter = 1 (bindings.cpp:29-33) */
    int64_t discrete_y;
    float start_x;               /* GridState.startX/Y (ball start, spawn centre) */
    float start_y;
    int64_t max_episode_length;  /* accepted and ignored, as in the reference */
    int32_t exec_mode;           /* BB_EXEC_CPU or BB_EXEC_CUDA */
    int32_t gpu_id;              /* -1: current device */
    int64_t num_worlds;          /* worlds owned by this simulator (this rank's shard) */
    int64_t world_offset;        /* global index of local world 0 (sharding) */
    uint32_t rand_seed;          /* reference hard-codes 0 (bindings.cpp:37) */
    uint32_t flags;              /* BB_FLAG_* */
    int32_t num_agents;          /* 2 = the reference game; 4 and 10 = extensions */
    int32_t reserved;
} bb_config;

/* Fill *cfg with the reference defaults (scripts/env.py:20-35 constructor). */
int bb_default_config(bb_config *cfg);

/* Observation row width for num_agents (128 at 2 agents, src/types.hpp:166). */
int32_t bb_obs_width(int32_t num_agents);

/* Bytes of buffer `export_id` for cfg (caller-owned storage path). */
int bb_buffer_bytes(const bb_config *cfg, int32_t export_id, int64_t *bytes);

/* Create a simulator that allocates and owns all of its buffers. */
int bb_create(const bb_config *cfg, bb_sim **out);

/* Create a simulator over caller-owned buffers: bufs[id] for every id in
 * [0, BB_NUM_REFERENCE_EXPORTS) and [BB_INTERNAL_FIRST, BB_INTERNAL_LAST]
 * (nbuf = BB_INTERNAL_LAST + 1, unused slots NULL), each at least
 * bb_buffer_bytes() long, 16-byte aligned, on the simulator's device (host
 * memory in CPU mode).  Worlds are generated into them (src/gen.cpp:13-214). */
int bb_create_with_buffers(const bb_config *cfg, void *const *bufs, int32_t nbuf, bb_sim **out);

int bb_destroy(bb_sim *sim);

/* One step of every world (the task graph of src/game.cpp:1463-1526),
 * asynchronous on `stream` in CUDA mode, synchronous in CPU mode. */
int bb_step(bb_sim *sim, void *stream);

/* n steps.  If random_actions != 0, each step first overwrites the action
 * tensor with the synthetic workload threefry2x32(key={action_seed, step0+s},
 * ctr={global world, agent}) (buckets [2,8,3,2,2,2], scripts/env.py:102).
 * If kernel_ms is non-NULL (CUDA mode), HIP events bracket every step kernel
 * and the summed kernel time is written there after a stream sync. */
int bb_step_n(bb_sim *sim, int32_t n, int32_t random_actions, uint32_t action_seed,
              uint32_t step0, void *stream, float *kernel_ms);

/* Only the synthetic action write (the bench's stand-in for the Python
 * `actions[:] = ...` write of scripts/env.py:147). */
int bb_write_random_actions(bb_sim *sim, uint32_t action_seed, uint32_t step, void *stream);

/* n steps whose actions are already resident: step k reads its actions from
 * (and the defence AI writes its overrides back to) the int32 rows
 * actions + k * num_worlds * num_agents * 6 (layout [n][W][N][6], memory of the
 * simulator's device in CUDA mode, host memory in CPU mode) instead of the
 * action tensor; afterwards the action tensor holds step n-1's rows.
 * On gfx950 the n steps run as one launch, every step's outputs (each state
 * column, observation row, reward, done and action write-back) written as by
 * bb_step; identical results to n bb_step launches.  At 2 agents, and at
 * more while a step's bytes stay in the Infinity Cache, the worlds stay on
 * the chip between steps (registers: k_rollout_split / k_rollout; LDS from 4
 * agents: k_rollout_shared; BB_STAGED_RESIDENT); otherwise each wave steps its
 * worlds n times reloading the state its lanes stored (k_step_loop:
 * BB_STAGED_LOOP).  MADRONA_BB_STEP_LOOP = 0 / 1 / 2 forces one launch per
 * step / the reloading loop / the resident loop where it exists.
 * kernel_ms as in bb_step_n (the launch's). */
int bb_step_n_staged(bb_sim *sim, int32_t n, int32_t *actions, void *stream, float *kernel_ms);

/* The launch bb_step_n_staged makes for n steps on this simulator, and the
 * algorithmic bytes of that call over all worlds: n B(N) per world, less the
 * state reads of steps 1..n-1 on the resident path. */
#define BB_STAGED_PER_STEP 0 /* one step launch per step (also: CPU mode, n < 2) */
#define BB_STAGED_LOOP 1     /* one k_step_loop launch */
#define BB_STAGED_RESIDENT 2 /* one k_rollout_split / k_rollout launch, state columns stored every step */
int32_t bb_step_staged_path(const bb_sim *sim, int32_t n);
int64_t bb_step_staged_bytes(const bb_sim *sim, int32_t n);

/* Stage n steps of the synthetic workload of bb_step_n (steps step0..step0+n-1)
 * into actions[n][W][N][6] for bb_step_n_staged. */
int bb_fill_random_actions(bb_sim *sim, int32_t *actions, int32_t n, uint32_t action_seed, uint32_t step0,
                           void *stream);

/* bb_rollout flags */
#define BB_ROLLOUT_PER_STEP 0x1u /* one step kernel launch per step, state through HBM
                                    (default on gfx950 at 2 agents: one launch for all
                                    steps, the worlds held in registers) */

/* n-step rollout.  Equivalent to, for k = 0..n-1:
 *     action tensor := actions[k]; bb_step();
 *     obs_out[k] := observations; reward_out[k] := reward; done_out[k] := done
 * with the defence AI's overrides written back into actions[k] (as
 * bb_step_n_staged).  Layouts: actions int32 [n][W][N][6], obs_out float
 * [n][W][N][obs_width], reward_out/done_out float [n][W][N], on the
 * simulator's device (host memory in CPU mode).  Observation columns from
 * roundup4(61 + 38(N-1) + 2N) on are never written: zero obs_out once.  A
 * NULL output is not recorded (that tensor of the simulator is rewritten
 * every step instead).  Afterwards every simulator column holds the state
 * after step n-1 (observations, reward, done and action included).
 * kernel_ms as in bb_step_n (summed over the launches). */
int bb_rollout(bb_sim *sim, int32_t n, int32_t *actions, float *obs_out, float *reward_out, float *done_out,
               uint32_t flags, void *stream, float *kernel_ms);

/* Trajectory recorder.  One record of one world is bb_record_words(N) int32
 * words (18 N + 27): the columns scripts/ppo.py:94-105 logs, in its key order
 * and each in its export layout -- agent_pos f32[N][3], ball_pos f32[3],
 * ball_vel f32[3], orientation f32[N][4], ball_physics i32[7],
 * agent_possession i32[N][3], game_state f32[14], reward f32[N],
 * action i32[N][6], done f32[N].  bb_record copies worlds [world0,
 * world0 + count) to dst + slot * count * words (records world-major), on
 * `stream` after whatever precedes it there; host memory in CPU mode. */
int32_t bb_record_words(int32_t num_agents);
int bb_record(bb_sim *sim, int64_t world0, int32_t count, int32_t *dst, int64_t slot, void *stream);

/* Policy inference (scripts/agent.py:108-154 at num_channels = 32,
 * num_layers = 2, input 128, buckets [2,8,3,2,2,2]).  fp32 row-major
 * [out][in] weights on the device (host memory for BB_EXEC_CPU); obs_inv =
 * rsqrt(running var + 1e-5) as agent.py:30-35 computes it; head_w / head_b =
 * the 19 actor rows, the critic row, then 12 zero rows (32 x 32, 32). */
typedef struct bb_policy_weights {
    const float *obs_mean, *obs_inv;
    const float *w1, *b1, *ln1_w, *ln1_b;
    const float *w2, *b2, *ln2_w, *ln2_b;
    const float *head_w, *head_b;
} bb_policy_weights;

/* For rows r in [0, rows): reads obs + r * obs_stride (128 floats, 16-byte
 * aligned), writes 6 int32 actions to actions + r * action_stride (e.g. the
 * action tensor's column of one agent), and optionally log_prob[r] (sum over
 * the buckets) and value[r].  stochastic = 0: per-bucket argmax (best(),
 * scripts/action.py:21-23); 1: a categorical sample (Categorical.sample,
 * action.py:29-33) by inverse CDF, bucket b's uniform from threefry({seed,
 * step}, {r, b >> 1}) word b & 1.  gpu_id: the device of the pointers (CUDA
 * mode). */
int bb_policy_forward(const bb_policy_weights *w, int32_t exec_mode, int32_t gpu_id, const float *obs,
                      int64_t rows, int64_t obs_stride, int32_t *actions, int64_t action_stride, float *log_prob,
                      float *value, int32_t stochastic, uint32_t seed, uint32_t step, void *stream);

/* bb_policy_forward at the observation widths of the 2v2 to 5v5 games: the
 * network Agent(envs.get_input_dim(), num_channels = 32, num_layers = 2)
 * builds (scripts/agent.py:108-124) when the simulator exports in_dim =
 * bb_obs_width(N) = 184, 264, 344 or 424 floats (N = 4, 6, 8, 10).  w as above
 * with obs_mean, obs_inv [in_dim] and w1 [32][in_dim].  Rows, outputs and
 * sampling as bb_policy_forward (reads in_dim floats at obs + r * obs_stride,
 * nothing behind them); actions may be NULL (log_prob / value only,
 * agent.evaluate, agent.py:168-170).  BB_ERR_INVALID_ARG for any other
 * in_dim, obs_stride < in_dim, a NULL weight or rows / w1 / w2 / head_w not
 * 16-byte aligned. */
int bb_policy_forward_wide(const bb_policy_weights *w, int32_t in_dim, int32_t exec_mode, int32_t gpu_id,
                           const float *obs, int64_t rows, int64_t obs_stride, int32_t *actions, int64_t act_stride,
                           float *log_prob, float *value, int32_t stochastic, uint32_t seed, uint32_t step,
                           void *stream);

/* PPO's rollout on the device (scripts/ppo.py:61-141 over scripts/env.py:126-170;
 * the reference's 2-agent game).  For k = 0..n-1:
 *     actions, log_probs, values = agent(obs)          (policy w, trainee rows)
 *     [opponent: the frozen policy acts for the other agent, env.py:127-143]
 *     actions[:, trainee] = actions; bb_step()          (env.py:147,155)
 *     buffer.obs/actions/log_probs/values[k] = obs, actions, log_probs, values
 *     buffer.rewards/dones[k] = the trainee's reward / done after the step
 * and then next_value = agent.evaluate(obs after the last step) (ppo.py:136-137).
 * Each output is optional (NULL: not recorded; reward and done together).
 * Layouts (the simulator's device, host memory in CPU mode): obs float [n][W][128],
 * actions int32 [n][W][6] (the policy's, before the defence AI's overrides),
 * log_prob / value / reward / done float [n][W], next_value float [W].
 * Sampling as bb_policy_forward with step = step0 + k (stochastic = 0: argmax);
 * the opponent samples with seed ^ 0x9E3779B9.  Equal, bit for bit, to n x
 * (bb_policy_forward on the trainee rows; bb_step) with the reads above.
 * On gfx950, up to 16 384 worlds one fused launch runs all n steps with the
 * worlds in registers (BB_PPO_PATH_FUSED_ROLLOUT), the opponent's network too
 * when there is one; above, one launch in which every wave runs the policy
 * pass of step 0 and then its worlds' n steps, each followed by the next
 * policy pass on the rows in LDS (BB_PPO_PATH_FUSED_STEP) -- with an opponent
 * the frozen network's pass too, on the other agent's rows in the same LDS
 * tile, so an opponent runs in the one launch at every world count.  flags
 * BB_ROLLOUT_PER_STEP forces a policy launch (two with an opponent) and a step
 * launch per step instead; from 32 768
 * worlds those per-step launches of two world halves go to `stream` and to a
 * second stream the simulator owns (created on first use, destroyed by
 * bb_destroy); `stream` waits for both before the call's last work, so stream
 * order holds for the caller.
 * kernel_ms (CUDA mode): time from the first launch to the last, after a sync. */
typedef struct bb_policy_rollout_buffers {
    float *obs;
    int32_t *actions;
    float *log_prob, *value, *reward, *done, *next_value;
} bb_policy_rollout_buffers;
int bb_rollout_policy(bb_sim *sim, const bb_policy_weights *w, const bb_policy_weights *opponent, int32_t n,
                      int32_t trainee, int32_t stochastic, uint32_t seed, uint32_t step0,
                      const bb_policy_rollout_buffers *out, uint32_t flags, void *stream, float *kernel_ms);

/* The implementation bb_rollout_policy takes on this simulator, and the
 * algorithmic bytes of one call of n steps with every output recorded (the
 * bytes that path must move: HBM roofline of the PPO loop).
 * On a simulator of other than 2 agents both fail: BB_ERR_UNSUPPORTED (< 0),
 * bb_last_error() says why. */
#define BB_PPO_PATH_HOST 0          /* CPU mode: the host executor */
#define BB_PPO_PATH_FUSED_ROLLOUT 1 /* one k_rollout_policy (opponent: k_rollout_selfplay) launch for all n steps */
#define BB_PPO_PATH_FUSED_STEP 2    /* one k_rollout_ppo launch: policy pass 0, then n x (step + next policy pass; opponent: both networks' passes) */
#define BB_PPO_PATH_PER_STEP 3      /* a policy launch and a step launch per step */
int32_t bb_rollout_policy_path(const bb_sim *sim, int32_t with_opponent, uint32_t flags);
int64_t bb_rollout_policy_bytes(const bb_sim *sim, int32_t with_opponent, uint32_t flags, int32_t n);

/* PPO's minibatch update up to param.grad (scripts/ppo.py:190-213 update_policy:
 * buffer.get_minibatch scripts/buffers.py:25-33, agent.get_stats
 * scripts/agent.py:172-178 over scripts/action.py:35-44, the clipped surrogate,
 * clipped value and entropy losses ppo.py:195-210 with clip_vloss, backward()):
 * forward, loss and backward of the policy network over the m minibatch rows
 * in one pass.  The batch is the rollout buffer's flat view: obs float
 * [rows][128] (16-byte aligned), actions int32 [rows][6], log_prob / value /
 * advantages / returns float [rows]; idx int64 [m] the minibatch's buffer rows
 * (mb_inds; NULL: rows 0..m-1), gathered by the kernel.  An index outside
 * [0, rows) contributes nothing.  Writes d loss / d parameter for the weights
 * `w` into `grads` (bb_policy_weights without the normaliser, whose statistics
 * are not parameters; head rows 0-18 the actor, 19 the critic, 20-31 zero) and
 * loss4 = {loss, pg_loss, c_loss before vf_coef, mean entropy}, with
 * loss = pg_loss + vf_coef c_loss - ent_coef entropy (ppo.py:206-210).
 * workspace: bb_policy_ppo_grad_workspace_bytes(m) bytes on the device,
 * 16-byte aligned (CUDA mode; unused in CPU mode, may be NULL there).  No
 * atomics: the same inputs give the same bits.  No synchronisation. */
typedef struct bb_ppo_batch {
    const float *obs;
    const int32_t *actions;
    const float *log_prob, *value, *advantages, *returns;
    const int64_t *idx;
    int64_t rows, m;
} bb_ppo_batch;
typedef struct bb_ppo_coef {
    float clip_coef, vf_coef, ent_coef;
} bb_ppo_coef;
typedef struct bb_policy_grads {
    float *w1, *b1, *ln1_w, *ln1_b;
    float *w2, *b2, *ln2_w, *ln2_b;
    float *head_w, *head_b;
} bb_policy_grads;
int bb_policy_ppo_grad(const bb_policy_weights *w, int32_t exec_mode, int32_t gpu_id, const bb_ppo_batch *batch,
                       const bb_ppo_coef *coef, bb_policy_grads *grads, float *loss4, void *workspace,
                       int64_t workspace_bytes, void *stream);
int64_t bb_policy_ppo_grad_workspace_bytes(int64_t m);

/* bb_policy_ppo_grad for the networks bb_policy_forward_wide serves: in_dim =
 * 184, 264, 344 or 424 inputs.  batch->obs is float [rows][in_dim] contiguous
 * (16-byte aligned; every width is a multiple of 8, so every row is), w->w1,
 * w->obs_mean / obs_inv and grads->w1 are [32][in_dim] / [in_dim]; everything
 * else as bb_policy_ppo_grad: the same loss, the same gathered rows, loss4, no
 * atomics, no synchronisation.  On gfx950 two passes over the minibatch rows
 * and a reduce: the first runs forward, loss and backward and leaves dloss/dz1
 * [m][32] in the workspace, the second multiplies it into dW1 against the
 * re-read rows.  workspace: bb_policy_ppo_grad_wide_workspace_bytes(in_dim, m)
 * bytes on the device, 16-byte aligned (CUDA mode; unused in CPU mode): the dz1
 * rows and both passes' partial sums; 0 for another in_dim or m <= 0.
 * BB_ERR_INVALID_ARG (nothing launched) for any other in_dim and for whatever
 * bb_policy_ppo_grad refuses. */
int64_t bb_policy_ppo_grad_wide_workspace_bytes(int32_t in_dim, int64_t m);
int bb_policy_ppo_grad_wide(const bb_policy_weights *w, int32_t in_dim, int32_t exec_mode, int32_t gpu_id,
                            const bb_ppo_batch *batch, const bb_ppo_coef *coef, const bb_policy_grads *grads,
                            float *loss4, void *workspace, int64_t workspace_bytes, void *stream);

/* PPO's phase between the rollout and the minibatch updates (scripts/ppo.py:144-177
 * compute_advantages over scripts/agent.py:28-50 RunningMeanStd), on the
 * buffers bb_rollout_policy filled: obs float [steps][worlds][128] (16-byte
 * aligned), value / reward / done float [steps][worlds], next_value float
 * [worlds].  With m = (float)value_norm.mean, s = (float)value_norm.var + 1e-5f:
 *   v = m + sqrt(s) clamp(value, +-5), nv likewise              (agent.py:31-34)
 *   GAE backwards over the steps, A and Rt = A + v              (ppo.py:153-166;
 *     the last step takes 1 - done[steps-1] as its non-terminal flag, ppo.py:157)
 *   obs_norm.update(obs rows), value_norm.update(v), value_norm.update(Rt)
 *     in this order, each from the batch mean and unbiased variance, merged in
 *     double in place                           (ppo.py:168-170, agent.py:41-50)
 *   advantages = (A - mu) / (sigma + 1e-8), mu / sigma the mean and unbiased
 *     std of A; returns = clamp((Rt - m') rsqrt(s'), +-5) with m', s' of the
 *     updated value_norm                                        (ppo.py:173-176)
 * `value` is not written (ppo.py:175 writes to a temporary).  out4 = {mu, sigma,
 * value_norm's new mean, new var}.  A bb_running_stats holds device (CUDA mode)
 * or host pointers to RunningMeanStd's double buffers: mean[dim], var[dim],
 * count[1], 8-byte aligned; dim 1 for value_norm, 128 for obs_norm.
 * steps x worlds >= 2.  workspace: bb_policy_advantages_workspace_bytes(steps,
 * worlds) bytes on the device, 16-byte aligned (CUDA mode; unused in CPU mode,
 * may be NULL there; 0 for a shape the entry refuses).  No atomics: the same
 * inputs give the same bits.  No synchronisation. */
typedef struct bb_running_stats {
    double *mean, *var, *count;
} bb_running_stats;
typedef struct bb_adv_batch {
    const float *obs, *value, *reward, *done, *next_value;
    float *advantages, *returns;
    int64_t steps, worlds;
} bb_adv_batch;
int bb_policy_advantages(int32_t exec_mode, int32_t gpu_id, const bb_adv_batch *batch,
                         const bb_running_stats *value_norm, const bb_running_stats *obs_norm, double gamma,
                         double gae_lambda, float *out4, void *workspace, int64_t workspace_bytes, void *stream);
int64_t bb_policy_advantages_workspace_bytes(int64_t steps, int64_t worlds);

/* bb_policy_advantages for observation rows of in_dim = 184, 264, 344 or 424
 * floats: batch->obs is float [steps][worlds][in_dim], obs_norm holds in_dim
 * statistics; everything else, every formula and every check as above.
 * workspace: bb_policy_advantages_wide_workspace_bytes(in_dim, steps, worlds)
 * bytes (0 for another in_dim).  BB_ERR_INVALID_ARG (nothing launched) for any
 * other in_dim. */
int bb_policy_advantages_wide(int32_t in_dim, int32_t exec_mode, int32_t gpu_id, const bb_adv_batch *batch,
                              const bb_running_stats *value_norm, const bb_running_stats *obs_norm, double gamma,
                              double gae_lambda, float *out4, void *workspace, int64_t workspace_bytes, void *stream);
int64_t bb_policy_advantages_wide_workspace_bytes(int32_t in_dim, int64_t steps, int64_t worlds);

/* What follows loss.backward() in one minibatch of update_policy
 * (scripts/ppo.py:214-215): torch.nn.utils.clip_grad_norm_, then
 * torch.optim.Adam's step with its defaults (no weight decay, no amsgrad),
 * then the new parameters into the packed weight image `w`, so that the next
 * bb_policy_ppo_grad / bb_policy_forward reads them.  Over all 5 972 elements:
 *   norm = |g|_2,  coef = min(1, max_grad_norm / (norm + 1e-6)),  g = g coef
 *   m = m + (1 - beta1)(g - m),  v = beta2 v + (1 - beta2) g g
 *   p = p - lr / (1 - beta1^t) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),  t = ++step
 * bb_policy_params: 12 float tensors in the order of Agent.parameters()
 * (`params`: the parameters, updated; `grads`: their .grad tensors, left
 * clipped as clip_grad_norm_ leaves them).  Packed rows: head_w rows 0-18 =
 * actor_w, row 19 = critic_w, rows 20-31 untouched (zero); likewise head_b.
 * A packed pointer may equal the parameter's pointer.  obs_mean / obs_inv are
 * not written.  bb_adam_state: exp_avg / exp_avg_sq float [5972] in the order
 * w1 b1 ln1_w ln1_b w2 b2 ln2_w ln2_b actor_w critic_w actor_b critic_b,
 * step int64 [1], ticket int32 [1] (CUDA mode; may be NULL in CPU mode), all
 * zero-initialised by the caller, on the device in CUDA mode; the ticket is 0
 * again after every call.
 *
 * bb_policy_adam_step: after any backward that filled `grads`.  out2 = {norm
 * before clipping, coef}.
 * bb_policy_ppo_step: bb_policy_ppo_grad's pass over the minibatch (same batch
 * and coef), then the step, in two launches; nothing else is written.  out6 =
 * {loss, pg_loss, c_loss, entropy, norm, coef}.  workspace:
 * bb_policy_ppo_step_workspace_bytes(m) bytes on the device, 16-byte aligned
 * (CUDA mode).  The same state and inputs give the same bits, and
 * bb_policy_ppo_step gives the bits of bb_policy_ppo_grad followed by
 * bb_policy_adam_step.  No synchronisation. */
typedef struct bb_policy_params {
    float *w1, *b1, *ln1_w, *ln1_b;
    float *w2, *b2, *ln2_w, *ln2_b;
    float *actor_w, *actor_b, *critic_w, *critic_b;
} bb_policy_params;
typedef struct bb_adam_state {
    float *exp_avg, *exp_avg_sq;
    int64_t *step;
    int32_t *ticket;
} bb_adam_state;
typedef struct bb_adam_hyper {
    double lr, beta1, beta2, eps, max_grad_norm;
} bb_adam_hyper;
int bb_policy_adam_step(const bb_policy_weights *w, int32_t exec_mode, int32_t gpu_id, const bb_policy_params *params,
                        const bb_policy_params *grads, const bb_adam_state *state, const bb_adam_hyper *hyper,
                        float *out2, void *stream);
int bb_policy_ppo_step(const bb_policy_weights *w, int32_t exec_mode, int32_t gpu_id, const bb_ppo_batch *batch,
                       const bb_ppo_coef *coef, const bb_policy_params *params, const bb_policy_params *grads,
                       const bb_adam_state *state, const bb_adam_hyper *hyper, float *out6, void *workspace,
                       int64_t workspace_bytes, void *stream);
int64_t bb_policy_ppo_step_workspace_bytes(int64_t m);

/* The same two entries for the networks of in_dim = 184, 264, 344 or 424
 * inputs (bb_policy_ppo_grad_wide's).  params->w1, grads->w1 and w->w1 are
 * [32][in_dim]; exp_avg / exp_avg_sq are float [E], E = 32 in_dim + 1876 (7764,
 * 10324, 12884, 15444), in the same tensor order: w1 first, every later offset
 * the 128-wide one plus 32 (in_dim - 128).  Same math, same checks, same
 * results (out2 / out6).  bb_policy_ppo_step_wide runs
 * bb_policy_ppo_grad_wide's two passes, then the step, and gives the bits of
 * bb_policy_ppo_grad_wide followed by bb_policy_adam_step_wide.  workspace:
 * bb_policy_ppo_step_wide_workspace_bytes(in_dim, m) bytes on the device,
 * 16-byte aligned (CUDA mode): bb_policy_ppo_grad_wide's, then the unclipped
 * gradient and the partial sums of squares; 0 for another in_dim or m <= 0.
 * The ticket is not used.  BB_ERR_INVALID_ARG (nothing launched) for any other
 * in_dim. */
int bb_policy_adam_step_wide(const bb_policy_weights *w, int32_t in_dim, int32_t exec_mode, int32_t gpu_id,
                             const bb_policy_params *params, const bb_policy_params *grads, const bb_adam_state *state,
                             const bb_adam_hyper *hyper, float *out2, void *stream);
int bb_policy_ppo_step_wide(const bb_policy_weights *w, int32_t in_dim, int32_t exec_mode, int32_t gpu_id,
                            const bb_ppo_batch *batch, const bb_ppo_coef *coef, const bb_policy_params *params,
                            const bb_policy_params *grads, const bb_adam_state *state, const bb_adam_hyper *hyper,
                            float *out6, void *workspace, int64_t workspace_bytes, void *stream);
int64_t bb_policy_ppo_step_wide_workspace_bytes(int32_t in_dim, int64_t m);

int bb_set_action(bb_sim *sim, int32_t world_idx, int32_t agent_idx, int32_t move_speed,
                  int32_t move_angle, int32_t rotate, int32_t grab, int32_t pass,
                  int32_t shoot, void *stream);

int bb_trigger_reset(bb_sim *sim, int32_t world_idx, void *stream);

/* Describe one export: data pointer (aliasing the live state), dtype and
 * reference shape (src/mgr.cpp:317-445; ndim <= 3, dims[ndim..3] = 0). */
int bb_export(bb_sim *sim, int32_t export_id, void **ptr, int32_t *dtype, int32_t *ndim,
              int64_t dims[4]);

/* Accessors. */
int64_t bb_num_worlds(const bb_sim *sim);
int32_t bb_num_agents(const bb_sim *sim);
int32_t bb_exec_mode(const bb_sim *sim);

/* Algorithmic HBM bytes moved by one step of one world (roofline). */
int64_t bb_algorithmic_bytes_per_world(int32_t num_agents);

/* 1 if bb_rollout runs as one fused launch (gfx950) for num_agents. */
int32_t bb_rollout_fused(int32_t num_agents);

/* Algorithmic HBM bytes of a fused rollout (roofline): per world
 * and step (action row in, observation row + reward + done out), and per
 * world and launch (the remaining state columns, in once and out once). */
int64_t bb_rollout_bytes_per_world_step(int32_t num_agents);
int64_t bb_rollout_state_bytes_per_world(int32_t num_agents);

/* Message for the last error on this thread ("" if none). */
const char *bb_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
