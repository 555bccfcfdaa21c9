/*
 * thrl.h -- C ABI of libthrl_hip.so: the MI355X (gfx950) implementation of the
 * iterated-pricing-game hot path of HakimNessah/th_rl.
 *
 * The reference has NO FFI / plugin layer: its boundary is the
 * Python duck-typed protocol that th_rl/trainer.py:46-70 drives.  Each entry
 * point below therefore cites the reference *Python* code it replaces.  All
 * pointers marked "device" are device (HBM) pointers owned by the caller
 * (e.g. torch tensors); the library allocates nothing persistent, never
 * throws, never exits; every function returns 0 on success or a negative
 * thrl_err, and thrl_last_error() gives a thread-local message.  Work is
 * enqueued on the caller's HIP stream (passed as void*, 0 = default stream)
 * and is asynchronous; the caller synchronises.
 *
 * Re-entrant and thread-safe: calls on different threads / streams / devices do
 * not share mutable state.  The only process-wide state is (i) the thread-local
 * error string, (ii) a read-only cache of per-device figures (CU count, LDS per
 * CU, resident waves per CU from hipDeviceProp_t), keyed by the HIP device id
 * and filled once per device under a lock, and (iii) the tuning knobs
 * THRL_WAVE_MAX_WAVES_PER_CU and THRL_GREEDY_EPS (measurement only: the epsilon
 * below which the greedy-regime variants of the fused kernel are launched;
 * results do not depend on it), read from the environment once per process
 * (per call: thrl_run.kernel = THRL_KERNEL_WAVE_PLAIN / THRL_KERNEL_WAVE_GREEDY).
 * Launch geometry and thrl_workspace_bytes() refer to the CURRENT HIP device of
 * the calling thread (hipSetDevice / torch.cuda.device).
 *
 * Plain C: no torch / HIP types in any signature.
 */
#ifndef THRL_H
#define THRL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THRL_ABI_VERSION 4          /* 2: per-game sweeps in thrl_qtable_init, thrl_mixed and the *_train entry points;
                                       3: thrl_build_info, THRL_KERNEL_WAVE_PLAIN / _GREEDY, replay rings [G][buf_len];
                                       4: the choice arrays of thrl_op_draws / thrl_op_sample_action are int32 (an int8
                                       buffer of a version-3 caller would be overrun fourfold) */
#define THRL_MAXA 8          /* max agents per game (reference configs use 2) */
#define THRL_MAX_EPISODES_PER_LAUNCH 32

typedef enum {
    THRL_OK = 0,
    THRL_ERR_BAD_CONFIG = -1,   /* shape / range error in thrl_cfg              */
    THRL_ERR_NULL = -2,         /* a required pointer is NULL                   */
    THRL_ERR_UNSUPPORTED = -3,  /* requested kernel cannot run this config      */
    THRL_ERR_HIP = -4,          /* HIP runtime error (message has the string)   */
    THRL_ERR_WORKSPACE = -5     /* workspace / replay memory too small          */
} thrl_err;

typedef enum {
    THRL_KERNEL_AUTO = 0,       /* fused wave kernel when eligible, else generic */
    THRL_KERNEL_GENERIC = 1,    /* one thread per game, tables in HBM, f32/f64  */
    THRL_KERNEL_WAVE = 2,       /* one wavefront per game, tables in LDS, f32 / f64 */
    /* The wave kernel has two code variants with IDENTICAL results: the plain one and the greedy-regime one
     * (per-episode composed greedy tables, cyclic segments as register recurrences); THRL_KERNEL_WAVE picks by
     * epsilon (the greedy one once every agent's epsilon <= 0.05).  These two ids pin the variant for one call
     * -- measurements and the parity tests that cover each variant in each regime.  _GREEDY fails with
     * THRL_ERR_UNSUPPORTED where no greedy variant exists (noise, sweeps, multi-episode training cycles). */
    THRL_KERNEL_WAVE_PLAIN = 3,
    THRL_KERNEL_WAVE_GREEDY = 4,
    /* one wavefront per game, tables in LDS, for 1-4 QTable agents with INDIVIDUAL state / action grids (any
     * nplayers and any QTable per agent: trainer.py:21-23): games (with or without env noise) whose replay buffers
     * train once per episode; the state is carried as the action tuple of the last step, or as explicit table rows
     * after a step with a redrawn intercept; per-game sweeps (thrl_buffers.sweep_*) are taken, an epsilon-schedule
     * sweep needs sweep_eps.  AUTO picks it where the two-agent wave kernel does not apply. */
    THRL_KERNEL_TUPLE = 5
} thrl_kernel;

/*
 * Game description.  One thrl_cfg == the JSON config blocks that
 * trainer.create_game() splats into the constructors (trainer.py:13-26):
 *   per agent  : QTable.__init__ kwargs           (agents.py:13-28)
 *   environment: NoisyPriceState.__init__ kwargs  (environments.py:5)
 */
typedef struct {
    int32_t n_games;                 /* G: games stepped in lockstep on this device      */
    int32_t n_agents;                /* N = environment.nplayers = len(agents)           */
    int32_t max_steps;               /* T = environment.max_steps                        */
    int32_t q_dtype;                 /* 0 = float32 tables, 1 = float64 tables           */
    double  env_a, env_b;            /* demand intercept / slope (environments.py:5)     */
    double  noise_prob;              /* environments.py:28                               */
    int32_t n_states[THRL_MAXA];     /* QTable `states`  (table has states+1 rows)       */
    int32_t n_actions[THRL_MAXA];    /* QTable `actions`                                 */
    int32_t min_memory[THRL_MAXA];   /* agents.py:26,60                                  */
    int32_t capacity[THRL_MAXA];     /* ReplayBuffer deque maxlen (buffers.py:12)        */
    double  max_state[THRL_MAXA];    /* agents.py:21,48                                  */
    double  gamma[THRL_MAXA], alpha[THRL_MAXA];
    double  eps_end[THRL_MAXA], eps_step[THRL_MAXA];
    double  act_lo[THRL_MAXA], act_hi[THRL_MAXA];   /* action_range                      */
} thrl_cfg;

/*
 * HBM layout (all game-major so one game's data is one contiguous slab):
 *   q        [G][stride]  stride = sum_i (n_states[i]+1)*n_actions[i]; agent i's
 *                         block starts at off_i = sum_{j<i} rows_j*A_j and is the
 *                         reference's `QTable.table` (agents.py:29) row-major.
 *   counter  [G][stride]  int32, `QTable.counter` (agents.py:45,76); may be NULL.
 *   state    [G]          float64 env state = last price (environments.py:36).
 *   replay_mem            opaque, thrl_replay_mem_bytes(); the ReplayBuffer
 *                         contents that survive between episodes (buffers.py).
 */
typedef struct {
    void*    q;                      /* device, f32 or f64 per cfg.q_dtype               */
    int32_t* counter;                /* device or NULL                                   */
    double*  state;                  /* device                                           */
    void*    replay_mem;             /* device, generic kernel only (may be NULL for WAVE)*/
    size_t   replay_mem_bytes;
    double*  reward_log;             /* device [n_episodes][N]: mean over the G games of
                                        rewards_log[e,:] (trainer.py:65); or NULL        */
    double*  action_log;             /* device [n_episodes][N] (trainer.py:66); or NULL  */
    double*  game_reward_log;        /* device [n_episodes][N][G] per-game rows; or NULL */
    double*  game_action_log;        /* device [n_episodes][N][G]; or NULL               */
    /* Per-game rows (either array may be given alone) are written by every kernel thrl_qtable_episodes launches:
     * the wave kernel (all variants: plain, greedy, noise, sweeps, multi-episode training cycles; f32 / f64), the
     * tuple kernel (1-4 agents, individual grids, noise, sweeps; f32 / f64) and the generic kernel, so asking for
     * them does not change which kernel AUTO picks.  Row [e][i][g] = game g's rewards_log[e, i] / actions_log[e, i]
     * (trainer.py:65-66).  The reference adds r/T (scaled/T) step by step; the wave and tuple kernels sum the
     * episode's rewards and divide by T once, and sum the steps' scaled/T over the episode as a wave reduction,
     * i.e. the same values up to rounding order: rtol 1e-12, the mean logs' contract.  The
     * generic kernel keeps the sequential per-step sums. */
    /* parity mode: the reference's recorded random draws, or NULL for Philox       */
    const double* inj_u;             /* device [n_episodes][T][N][G] random.uniform(0,1) (agents.py:81) */
    const int8_t* inj_choice;        /* device [n_episodes][T][N][G] random.choice idx   (agents.py:82); one byte, so the
                                        generic kernel's route is THRL_ERR_BAD_CONFIG under injection with an agent of
                                        more than 128 actions (the LDS kernels stop at 64); read unsigned, clamped */
    const double* inj_noise_u;       /* device [n_episodes][T][G]    (environments.py:28); NULL if noise_prob<=0 */
    const double* inj_noise_a;       /* device [n_episodes][T][G]    (environments.py:29) */
    void*    workspace;              /* device scratch, thrl_workspace_bytes()           */
    size_t   workspace_bytes;
    /* Per-game hyper-parameter sweeps (optional; NULL = thrl_cfg's scalar for every game): the
     * reference sweeps configs x runs one process at a time (main.py:13-21); here a sweep is a
     * per-game array.  Device, layout [N][G] (agent-major); honoured by both episode kernels. */
    const double* sweep_gamma;       /* QTable gamma  (agents.py:30)                     */
    const double* sweep_alpha;       /* QTable alpha  (agents.py:31)                     */
    const double* sweep_eps_end;     /* agents.py:37                                     */
    const double* sweep_eps_step;    /* agents.py:36                                     */
    double*       sweep_eps;         /* in/out: current epsilon per (agent, game); when given it
                                        replaces thrl_run.eps (agents.py:35,78)          */
    const double* sweep_noise_prob;  /* device [G]; thrl_cfg.noise_prob must be > 0 if any entry is */
} thrl_buffers;

/* Host-side run state that is identical for every game (so it never lives in HBM). */
typedef struct {
    uint64_t seed;                   /* Philox key                                       */
    uint64_t game_offset;            /* global id of local game 0 (sharding-invariant RNG)*/
    uint64_t first_episode;          /* global episode index of the first episode        */
    int32_t  n_episodes;             /* episodes to run in this call                     */
    int32_t  kernel;                 /* thrl_kernel                                      */
    double   eps[THRL_MAXA];         /* in/out: QTable.epsilon (agents.py:35,78)         */
    int32_t  mem_count[THRL_MAXA];   /* in/out: appends since the last memory.empty();
                                        len(agent.memory) == min(mem_count, capacity)
                                        (buffers.py:12-19,40); kept in [0, 2*capacity)   */
    int32_t  kernel_used;            /* out: thrl_kernel actually launched               */
} thrl_run;

int         thrl_version(void);
const char* thrl_last_error(void);
/* What this binary is: "abi=4;ablate=<mask>;src=<hash of all kernel sources>;wave=<hash of the sources of the
 * headline kernel>;nn=<hash of the neural-agent kernels' sources>".  ablate != 0 marks a
 * TIMING-ONLY diagnostic build (phases of the fused kernel compiled out, results wrong by construction;
 * profiles/ablate.py) -- callers that report results or throughput must refuse it (bench.py does). */
const char* thrl_build_info(void);
/* the ablation mask alone (0 = the product library) */
int         thrl_ablate_mask(void);

/* elements per game in q / counter (sum_i rows_i*A_i); 0 on bad config */
size_t thrl_table_stride(const thrl_cfg* cfg);
/* element offset of agent i's table inside one game's slab */
size_t thrl_table_offset(const thrl_cfg* cfg, int agent);
size_t thrl_replay_mem_bytes(const thrl_cfg* cfg);
/* scratch the episode kernels need for THIS config on the current device (payoff LUT image, per-wave
 * log partials and transition log of the wave kernel's persistent grid; LUT image and per-wave visit log
 * of the tuple-chain kernel's); 0 on a bad config */
size_t thrl_workspace_bytes(const thrl_cfg* cfg);
/* which kernel THRL_KERNEL_AUTO would pick for this config (thrl_kernel) */
int    thrl_select_kernel(const thrl_cfg* cfg, int injected);
/* Host-only query: 1 when a launch of the wave kernel's plain float32 variant on this config builds its play tables in
 * closed form -- on the payoff grid the next row (float32 and float64 encode alike) is the local row
 * c - m0 * a0 - m1 * a1 for every action pair, and the config is noise-free with float32 tables, at most 62 reachable
 * rows and one episode per training cycle; 0 otherwise (the payoff look-up table is used).  Same results either way.
 * The answer is about the config: calls that run the GREEDY or a sweep variant, and the timing-only ablation builds
 * (thrl_ablate_mask() != 0), use the look-up table whatever it says.
 * out_c_m0_m1 (may be NULL) receives c, m0, m1 when the answer is 1. */
int    thrl_wave_play_form(const thrl_cfg* cfg, int out_c_m0_m1[3]);
/* Training cycle of the wave kernel: the replay buffers (buffers.py:12-19) reach min_memory every k-th
 * episode (agents.py:60), k = ceil(min_memory / max_steps); a call runs on the wave kernel when its
 * n_episodes is a multiple of k and the buffers are empty on entry (thrl_run.mem_count == 0), otherwise on
 * the generic kernel, which keeps the buffers in replay_mem.  Returns k >= 1, or 0 when the config is the
 * generic kernel's anyway. */
int    thrl_training_cycle(const thrl_cfg* cfg);

/*
 * Replaces QTable.__init__ table/counter init (agents.py:29,45) and
 * NoisyPriceState.reset() (environments.py:50-53, called once at trainer.py:45)
 * for all G games: q = 12.5/(1-gamma_i) + N(0,1), counter = 0, state ~ U(0,a),
 * from Philox4x32-10 keyed by (seed, global game id).  sweep_gamma: device [N][G] per-game gamma
 * (the table offset of a config sweep) or NULL for thrl_cfg.gamma.
 */
int thrl_qtable_init(const thrl_cfg* cfg, void* q, int32_t* counter, double* state,
                     uint64_t seed, uint64_t game_offset, const double* sweep_gamma, void* stream);

/*
 * THE hot path: replaces the body of trainer.train_one's loop (trainer.py:46-70)
 * for `run->n_episodes` episodes of all G games: per step QTable.sample_action
 * (agents.py:80-89), QTable.scale (:51-57), NoisyPriceState.step
 * (environments.py:25-39), ReplayBuffer.append (buffers.py:18-19), the log
 * accumulation (trainer.py:65-66); per episode QTable.train_net
 * (agents.py:59-78) = ReplayBuffer.replay/empty + snapshot-TD + epsilon decay.
 */
int thrl_qtable_episodes(const thrl_cfg* cfg, const thrl_buffers* bufs, thrl_run* run,
                         void* stream);

/*
 * Greedy evaluation rollout, replaces utils.play_game (utils.py:27-47):
 * env.reset() then `iters` episodes of get_action (agents.py:91-92) / scale /
 * env.step with no learning.  state0 [iters][G] are the reset() draws
 * (device, or NULL to draw from Philox); outputs are per-game episode means
 * mean_reward/mean_action [iters][N][G] (device).
 */
int thrl_play_greedy(const thrl_cfg* cfg, const void* q, const double* state0,
                     int32_t iters, uint64_t seed, uint64_t game_offset,
                     double* mean_reward, double* mean_action, void* stream);

/*
 * Unfused, batched-over-games operator forms of the reference methods (same
 * argument meaning, one call = one reference call applied to G games).  They
 * exist so a caller that drives the step loop itself (the duck-typed protocol)
 * still runs on the device.
 */
/* QTable.sample_action / get_action for agent `agent` (agents.py:80-92):
 * u device [G] f64, choice device [G] int32 (u==NULL => greedy get_action); price device [G];
 * encode32 != 0 applies the trainer's float32 cast first (trainer.py:53).  choice is int32 since ABI v4: an agent
 * may have 32,000 actions, and a byte wrapped every choice of 128 and more.  A choice outside [0, n_actions) is
 * device data the host cannot see: it is clamped to the last action (the rule of the injected choices below), so
 * a bad caller array cannot make the following thrl_op_td_update index outside the table. */
int thrl_op_sample_action(const thrl_cfg* cfg, int agent, const void* q, const double* price,
                          double eps, const double* u, const int32_t* choice, int encode32,
                          int32_t* action_out, void* stream);
/* QTable.encode for agent `agent` (agents.py:47-49): price [G] f64 -> row index [G] int32;
 * as_float32 != 0 evaluates it on the float32-cast state as sample_action does (trainer.py:53). */
int thrl_op_encode(const thrl_cfg* cfg, int agent, const double* price, int as_float32,
                   int32_t* row_out, void* stream);
/* QTable.scale for agent `agent` (agents.py:51-57): action index [G] int32 -> scaled [G] f64 */
int thrl_op_scale(const thrl_cfg* cfg, int agent, const int32_t* action, double* scaled_out, void* stream);
/* NoisyPriceState.step for G games (environments.py:25-39): scaled device [N][G] f64 = the
 * `actions` argument of the reference (already scaled); noise_u/noise_a device [G] or NULL
 * (the two numpy.random.uniform draws of :28-29); outputs price [G], reward [N][G]. */
int thrl_op_env_step(const thrl_cfg* cfg, const double* scaled, const double* noise_u,
                     const double* noise_a, double* price_out, double* reward_out, void* stream);
/* QTable.train_net's table update for agent `agent` on n transitions per game
 * (agents.py:61-76): price/next_price [n][G] f64, action [n][G] int32, reward [n][G] f64;
 * scratch: device [n][G] f64 (holds the old_value snapshot of agents.py:67). */
int thrl_op_td_update(const thrl_cfg* cfg, int agent, void* q, int32_t* counter, int32_t n,
                      const double* price, const int32_t* action, const double* reward,
                      const double* next_price, double* scratch, void* stream);

/*
 * Neural policy agent `Reinforce` (agents.py:119-220): a 1 -> 256 -> A MLP per game.
 * Parameter vector per game, P = thrl_nn_param_count(A) floats:
 *   [fc1.weight (256) | fc1.bias (256) | fc_pi.weight (A x 256 row-major) | fc_pi.bias (A)]
 * All arrays are device pointers and game-major: [G][P] for parameters and Adam moments, [G][ld] for the replayed
 * buffer (row g = game g's transitions in insertion order, the first n of its ld entries; ABI v3 -- v2 was
 * transition-major [n][G], which put one game's batch 8*G bytes apart: one 64-byte sector per transition).
 * float32 arithmetic as in torch.
 */
#define THRL_NN_HIDDEN 256
#define THRL_NN_MAX_TRANSITIONS 1400
size_t thrl_nn_param_count(int n_actions);
/* torch.nn.Linear default init, U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weights and biases
 * (agents.py:136-137), from Philox keyed by (seed, global game id, agent). */
int thrl_nn_init(int n_games, int n_actions, float* params, uint64_t seed, uint64_t game_offset,
                 int agent, void* stream);
/* Reinforce.pi + sample_action / get_action (agents.py:147-168) for G games: price [G] f64
 * (cast to float32 as the trainer does, trainer.py:53); u [G] uniforms in [0,1) for the
 * categorical draw (inverse CDF), or NULL for the greedy get_action; outputs action [G] and
 * optionally the probabilities [G][A]. */
int thrl_nn_act(int n_games, int n_actions, const float* params, const double* price, const double* u,
                int32_t* action_out, float* prob_out, void* stream);
/* Reinforce.train_net's update (agents.py:171-193) for G games on n replayed transitions each:
 * discounted returns, z-score (unbiased std), policy-gradient + entropy loss, gradient-norm clip
 * at 1.0, one Adam step (lr, betas 0.9/0.999, eps 1e-8).  step = Adam step count BEFORE the call.
 * price / action / reward: device [G][ld], n <= ld valid entries per row (a replay ring of thrl_mixed can be
 * passed as it is: ld = buf_len).  sweep_gamma / sweep_entropy: device [G] per-game values (a config sweep as
 * one batch) or NULL for the scalars.  grad_out [G][P] (optional) receives the clipped gradient.  returns_scratch
 * (optional): device [G][ld] floats; when given, the discounted returns (:178-181: a serial recurrence per game) are computed
 * by a pre-pass with one lane per game instead of by one thread of each game's block -- the same operations in the same
 * order, so the same bits; NULL keeps the in-kernel form. */
int thrl_nn_reinforce_train(int n_games, int n_actions, float* params, float* adam_m, float* adam_v,
                            int32_t step, int32_t n, int32_t ld, const double* price, const int32_t* action,
                            const double* reward, double gamma, double entropy_coef, double lr,
                            const double* sweep_gamma, const double* sweep_entropy,
                            float* grad_out, float* returns_scratch, void* stream);
/*
 * `ActorCritic` (agents.py:222-330): Reinforce's network plus a value head fc_v (256 -> 1, bias
 * initialised to 1000, :243-244) on the shared hidden layer.  Parameter vector per game,
 * thrl_ac_param_count(A) = thrl_nn_param_count(A) + 257 floats:
 *   [Reinforce layout | fc_v.weight (256) | fc_v.bias (1)]
 * thrl_ac_act = pi + sample_action / get_action (:262-272, identical to Reinforce's).
 * thrl_ac_train = train_net (:274-305) AS THE REFERENCE EXECUTES IT: `rewards` is [N] while v and
 * v_prime are [N,1], so advantage = (rewards + gamma*v_prime) - v broadcasts to [N,N]
 * (advantage[i,j] = r_j + gamma*v'_i - v_i); loss = mean_ij(advantage^2 - log p_j(a_j)*advantage)
 * + entropy_coef * (-mean H); v_prime is not detached.  next_price [G][ld] = the replayed new_state.
 */
size_t thrl_ac_param_count(int n_actions);
int thrl_ac_init(int n_games, int n_actions, float* params, uint64_t seed, uint64_t game_offset,
                 int agent, void* stream);
int thrl_ac_act(int n_games, int n_actions, const float* params, const double* price, const double* u,
                int32_t* action_out, float* prob_out, void* stream);
int thrl_ac_train(int n_games, int n_actions, float* params, float* adam_m, float* adam_v,
                  int32_t step, int32_t n, int32_t ld, const double* price, const int32_t* action,
                  const double* reward, const double* next_price, double gamma, double entropy_coef,
                  double lr, const double* sweep_gamma, const double* sweep_entropy, float* grad_out, void* stream);
/*
 * `CAC`, the continuous actor-critic (agents.py:333-442): fc1 (1 -> 256) and three 256 -> 1 heads,
 * mu = 4*tanh(fc_mu h), std = softplus(fc_std h), v = fc_v h.  THRL_CAC_PARAMS floats per game:
 *   [fc1.weight 256 | fc1.bias 256 | fc_mu.weight 256 | fc_mu.bias | fc_std.weight 256 | fc_std.bias |
 *    fc_v.weight 256 | fc_v.bias]
 * thrl_cac_act = pi + sample_action (:360-381): a = mu + std*z, z from u1,u2 [G] by Box-Muller,
 *   action = sigmoid(a) in (0,1) (float32 [G]); scale is action*(hi-lo)+lo (:371-375).
 *   u1 == NULL gives the MEAN action sigmoid(mu): the reference's get_action (:383-387) builds
 *   Normal(mu, 0), which torch rejects (ValueError, recorded in tests/golden/g9_cac.npz), so its play
 *   path cannot run; the mean action is what it intends.  mu/std/v outputs are optional.
 * thrl_cac_train = train_net (:389-416) AS THE REFERENCE EXECUTES IT: rewards / actions [N] against
 *   mu / std / v [N,1] broadcast to [N,N] -- advantage[i,j] = r_j + gamma*v'_i - v_i and
 *   log_prob[i,j] = log N(logit(a_j); mu_i, std_i); loss = mean_ij(advantage^2 - log_prob*advantage)
 *   + entropy_coef*(-mean entropy); clip 1.0; Adam.  action [G][ld] float32 as stored by the trainer.
 */
#define THRL_CAC_PARAMS 1283
int thrl_cac_init(int n_games, float* params, uint64_t seed, uint64_t game_offset, int agent, void* stream);
int thrl_cac_act(int n_games, const float* params, const double* price, const double* u1, const double* u2,
                 float* action_out, float* mu_out, float* std_out, float* v_out, void* stream);
int thrl_cac_train(int n_games, float* params, float* adam_m, float* adam_v, int32_t step, int32_t n, int32_t ld,
                   const double* price, const float* action, const double* reward, const double* next_price,
                   double gamma, double entropy_coef, double lr, const double* sweep_gamma, const double* sweep_entropy,
                   float* grad_out, void* stream);
/*
 * Fused episodes for games whose agents are any mix of QTable and Reinforce (the pairing of the
 * reference's example configs): trainer.train_one's loop (trainer.py:46-70) with QTable.train_net
 * inside the kernel.  Reinforce / ActorCritic transitions go to that agent's replay buffer; the
 * CALLER runs thrl_nn_reinforce_train / thrl_ac_train when len(memory) >= min_memory and must size n_episodes so that no
 * network update falls inside one call.  Replay buffers are rings [G][buf_len] per agent (game-major since ABI v3:
 * the 16-step flushes of the kernel and a game's whole batch in the update kernels are contiguous).
 */
typedef struct {
    int32_t kind[THRL_MAXA];             /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic, 3 = CAC */
    const float* nn_params[THRL_MAXA];   /* device [G][P] for the neural agents              */
    double*  buf_price[THRL_MAXA];       /* device [G][buf_len] state  (trainer.py:62)       */
    int32_t* buf_action[THRL_MAXA];      /* CAC agents: the float32 action's bits             */
    double*  buf_reward[THRL_MAXA];
    double*  buf_nprice[THRL_MAXA];      /* next state                                       */
    double*  buf_scratch[THRL_MAXA];     /* QTable agents: old_value snapshot (agents.py:67) */
    int32_t  buf_len[THRL_MAXA];
    int32_t  min_memory[THRL_MAXA];
    int32_t  count[THRL_MAXA];           /* in/out: appends since the last memory.empty()    */
    /* per-game sweeps of the QTable agents and the env, as in thrl_buffers: device [N][G] (noise_prob
     * [G]) or NULL.  Rows of neural agents are ignored here (their gamma / entropy sweep goes to the
     * *_train calls). */
    const double* sweep_gamma;
    const double* sweep_alpha;
    const double* sweep_eps_end;
    const double* sweep_eps_step;
    double*       sweep_eps;             /* in/out: current epsilon per (agent, game)        */
    const double* sweep_noise_prob;
    /* Optional scratch for the POLICY TABLE (ABI v3): inside one call the networks are frozen and, in a game
     * whose agents are all discrete, the state after a step is a function of that step's action tuple, so the
     * kernel evaluates Reinforce.pi / ActorCritic.pi (agents.py:147-152) once per call and tuple and looks the
     * result up afterwards (identical bits).  Device, thrl_mixed_policy_table_bytes() bytes, contents need not
     * survive between calls; NULL = evaluate the policy at every step (same results, slower). */
    float*   policy_tab;
    size_t   policy_tab_bytes;
    int32_t  flags;                      /* THRL_MIXED_* */
    /* Parity mode (optional; all five NULL = Philox draws and sampled neural play): the reference's recorded draws
     * and sampled actions, for the run->n_episodes episodes of this call.  inj_u / inj_choice / inj_noise_u /
     * inj_noise_a have the meaning and layout of the fields of thrl_buffers; inj_action is the action index a
     * Reinforce / ActorCritic agent's sample_action returned at that step (agents.py:160-163, 270-273), so the
     * float32 rounding of the policy cannot fork the trajectory: prices, rewards, replay rings and the QTable
     * agents' tables and counters are then the reference's exactly, both fused kernels skip the policy (the update
     * kernels recompute it from the replayed buffer).  Entries of inj_u / inj_choice that belong to a neural agent
     * and entries of inj_action that belong to a QTable agent are not read.
     * All or nothing: every stream the game consumes must be given -- inj_u and inj_choice with a QTable agent in
     * the game, inj_action with a Reinforce / ActorCritic agent, inj_noise_u and inj_noise_a with
     * cfg.noise_prob > 0 -- otherwise THRL_ERR_BAD_CONFIG.  An injected choice or action outside [0, n_actions) is
     * device data the host cannot see: it is clamped to the last action (thrl_crossplay's rule for policy entries),
     * nothing is read or written out of bounds.  inj_choice is one byte per draw: a QTable agent of more than 128 actions
     * is THRL_ERR_BAD_CONFIG under injection.  A game with a CAC agent is THRL_ERR_UNSUPPORTED under injection:
     * its action is a float, and the reference's play path for it cannot run (see thrl_cac_act).  Per-game sweeps
     * combine with injection as in thrl_qtable_episodes. */
    const double* inj_u;                 /* device [n_episodes][T][N][G] random.uniform(0,1) (agents.py:81)   */
    const int8_t* inj_choice;            /* device [n_episodes][T][N][G] random.choice idx   (agents.py:82)   */
    const double* inj_noise_u;           /* device [n_episodes][T][G]    (environments.py:28)                 */
    const double* inj_noise_a;           /* device [n_episodes][T][G]    (environments.py:29)                 */
    const int8_t* inj_action;            /* device [n_episodes][T][N][G] Categorical.sample().item()          */
} thrl_mixed;
/* Two-agent games whose neural agents are discrete run on the tuple-chain kernel (the state is carried as the action pair of
 * the last step, or as its price after a step with a redrawn intercept; needs policy_tab; per-game sweeps are taken): same
 * results as the general kernel.  This flag keeps the general one.  Any run->n_episodes is taken in ONE launch: that
 * kernel counts a launch's visits in 16-bit cells and folds them into `counter` every floor(65535 / max_steps) episodes
 * (max_steps <= 256 there), so the counters are exact however many visits one cell gets. */
#define THRL_MIXED_NO_TUPLE_KERNEL 1
/* bytes of thrl_mixed.policy_tab this configuration can use on this many games (0: the table does not apply --
 * no discrete neural agent, a continuous agent in the game, more than 2,048 action tuples, or a price grid small
 * enough for the in-LDS memo) */
size_t thrl_mixed_policy_table_bytes(const thrl_cfg* cfg, const thrl_mixed* mx);
int thrl_mixed_episodes(const thrl_cfg* cfg, thrl_mixed* mx, void* q, int32_t* counter, double* state,
                        thrl_run* run, double* game_reward_log, double* game_action_log, void* stream);

/* Philox draws for one lockstep step of a caller-driven loop: u [N][G] f64 uniforms and
 * choice [N][G] int32 indices in [0, n_actions[i]) (agents.py:81-82; int8 before ABI v4), optionally u2 [N][G] (the word behind `choice` as a
 * uniform: CAC's second Box-Muller input) and the env's two noise draws [G]
 * (environments.py:28-29); same streams/counters as thrl_qtable_episodes uses internally. */
int thrl_op_draws(const thrl_cfg* cfg, uint64_t seed, uint64_t game_offset, uint64_t episode, int32_t step,
                  double* u_out, int32_t* choice_out, double* u2_out, double* noise_u_out, double* noise_a_out,
                  void* stream);

/*
 * Per-group statistics of per-game episode rows: the distribution over replicas that the reference's analysis
 * plots per config (utils.py plot_learning_curve_conf / plot_learning_curve_sweep: median and 25th / 75th
 * percentile over runs of the total reward per epoch; plot_sweep_conf / plot_mean_conf: the same for greedy play).
 * Input: the rows thrl_qtable_episodes / thrl_mixed_episodes / thrl_play_greedy write, [E][N][G] float64, and a
 * group per game.  Q = 2N+1 quantities per game and episode, in this order: reward_i (i < N), action_i (i < N),
 * total = sum_i reward_i (added in agent order, float64).
 *
 * Outputs are ACCUMULATED (+= / max) into caller-zeroed device arrays, cell [e][group][q]:
 *   hist   uint32 [E][n_groups][Q][B+2]  bin 0 = x < lo_q, bin B+1 = x >= hi_q or x not finite, bin b in 1..B =
 *          1 + min(B-1, (int)floor((x - lo_q) * inv_w_q)) for lo_q <= x < hi_q (two roundings: subtract, multiply).
 *   sums   int64  [E][n_groups][Q][2]    sum of rint(xc * s1_q) and of rint((xc*xc) * s2_q), xc = x clamped to
 *          [-M_q, M_q], M_q = 16 * max(|lo_q|, |hi_q|).  s1_q, s2_q are powers of two chosen by the caller with
 *          s1_q * M_q * n_max <= 2^62 and s2_q * M_q^2 * n_max <= 2^62 for n_max the largest group over ALL the
 *          calls whose outputs will be added (every shard of a run): then no partial sum can overflow an int64.
 *          The library checks the bound for this call's n_games.  Sums are exact for |x| <= M_q; a value beyond
 *          enters them as +-M_q (its bin and min / max stay exact).  Non-finite values count in bin B+1 only.
 *   minmax uint64 [E][n_groups][Q][2]    [0] = ~key(min x), [1] = key(max x), key(x) = order-preserving image of
 *          the double's bits (sign bit clear: bits | 2^63; set: ~bits), combined by atomic max; 0 = no finite value.
 * Everything is integer, so the result is bit-identical for any launch geometry, any cut of the episodes into
 * calls and any split of the games into shards whose outputs are combined afterwards (hist and sums added,
 * minmax by element-wise max).
 *
 * Grouping: group_of (HOST, [G]) is validated here; perm / seg_off (device) are its stable sort -- local games in
 * group order, group k at perm[seg_off[k] .. seg_off[k+1]).  Each block works inside one group at a time and keeps
 * a private LDS histogram (B+2 words).  The kernel never reads or writes outside its arrays whatever perm /
 * seg_off hold (out-of-range entries are skipped), but only their stable sort of group_of gives the statistics.
 */
#define THRL_STATS_MAX_BINS 1024
#define THRL_STATS_MAXQ (2 * THRL_MAXA + 1)
typedef struct {
    int32_t n_games;                 /* G: columns of the rows                           */
    int32_t n_agents;                /* N                                                */
    int32_t n_episodes;              /* E: rows                                          */
    int32_t n_groups;
    int32_t n_bins;                  /* B in 1..THRL_STATS_MAX_BINS                      */
    int32_t reserved;                /* 0                                                */
    const double*  game_reward_log;  /* device [E][N][G]                                 */
    const double*  game_action_log;  /* device [E][N][G]                                 */
    const int32_t* group_of;         /* HOST [G], each in [0, n_groups)                  */
    const int32_t* perm;             /* device [G]                                       */
    const int64_t* seg_off;          /* device [n_groups + 1]                            */
    double lo[THRL_STATS_MAXQ], hi[THRL_STATS_MAXQ];    /* histogram range per quantity, hi > lo          */
    double inv_w[THRL_STATS_MAXQ];   /* B / (hi - lo), computed by the caller in double  */
    double scale[THRL_STATS_MAXQ][2];/* s1, s2 per quantity                              */
    uint32_t* hist;                  /* device outputs, see above                        */
    int64_t*  sums;
    uint64_t* minmax;
} thrl_group_stats_args;
int thrl_group_stats(const thrl_group_stats_args* args, void* stream);

/*
 * Exponentially weighted mean of per-game episode rows, carried across calls: the smoothing the reference applies to
 * each run's learning curve before it takes statistics over runs (utils.py:20-21 load_experiment, and
 * plot_learning_curve_conf / plot_learning_curve_sweep: log[...].ewm(halflife=1000).mean(), pandas' adjust=True
 * form).  The smoothed rows keep the episode-row layout, so thrl_group_stats reduces them as they are; its "total" is
 * then the sum of the smoothed rewards in agent order, the reference's .ewm().mean().sum(axis=1).
 *
 * Definition, float64, every operation rounded once (no fma).  The caller computes alpha = 1 - exp(log(0.5) / halflife)
 * and decay = 1 - alpha in double, in that order.  For row t = 0, 1, ... since the state was fresh, each of the 2N
 * state rows j (reward_0..reward_{N-1}, action_0..action_{N-1}) and each game g:
 *   num_t = x_t + decay * num_{t-1}    (num_{-1} = 0; the product is rounded, then the sum)
 *   den_t = 1   + decay * den_{t-1}    (den_{-1} = 0; the same for every game, so it is a host double)
 *   y_t   = num_t / den_t
 * The loop over the rows is sequential in every thread, so the result is bit-identical however the rows are cut into
 * calls: pass state_out and *den_out of one call as state_in and den of the next.  A non-finite x makes that game's
 * num non-finite from then on (pandas skips a NaN; this does not); thrl_group_stats counts such values in its
 * overflow bin.
 *
 * One thread per (state row, game), lanes consecutive in g; the cost is one read and one write of the rows.
 * n_episodes = 0 is accepted after the checks and does nothing: no array is read or written and *den_out = den.
 * Each output may be exactly its input (in place); any other overlap between an output and an input or another
 * output is refused, as is a state_out that overlaps state_in without being equal to it.
 */
typedef struct {
    int32_t n_games;                 /* G: columns of the rows, >= 1                     */
    int32_t n_agents;                /* N in 1..THRL_MAXA                                */
    int32_t n_episodes;              /* E: rows of this call, >= 0                       */
    int32_t reserved;                /* 0                                                */
    double decay;                    /* in (0, 1)                                        */
    double den;                      /* denominator before the first row: finite, >= 0; 0 = fresh */
    const double* reward_rows;       /* device [E][N][G]                                 */
    const double* action_rows;       /* device [E][N][G]                                 */
    double* reward_out;              /* device [E][N][G]; may be reward_rows             */
    double* action_out;              /* device [E][N][G]; may be action_rows             */
    const double* state_in;          /* device [2N][G]: num before the first row; NULL = zeros */
    double* state_out;               /* device [2N][G]: num after the last row; may be state_in */
    double* den_out;                 /* HOST, optional: denominator after the last row   */
} thrl_ewm_rows_args;
int thrl_ewm_rows(const thrl_ewm_rows_args* args, void* stream);

/*
 * Deviation analysis of the greedy policies (the test of Calvano, Calzolari, Denicolo, Pastorello, "Artificial
 * Intelligence, Algorithmic Pricing, and Collusion", AER 2020).  No reference counterpart: it extends
 * utils.play_game (utils.py:27-47).  QTable agents only; q, and everything else of the batch, is left untouched.
 * Every [.][G] array here has G = args.n_games: the first n_games games of q (n_games <= cfg.n_games).
 *
 * Greedy map F on row tuples x = (row_0 .. row_{N-1}): agent i plays a_i = argmax_row of its row x_i (first maximum
 * under strict >), then scale_action and env_step with NO env noise (intercept env_a) give the price p and the
 * rewards, and F(x)_i = encode64(p) (QTable.encode on the float64 price, as utils.play_game calls it).  The reward
 * and scaled action "at x" are those of the transition taken at x.
 *
 * Start state x_0 = encode64(state0[g]) per agent.  Pre-shock cycle: mu >= 0, lam >= 1 the smallest values with
 * x_{mu+lam} = x_mu.  The cycle is found iff mu + lam <= H (horizon); then s* = x_mu.  Otherwise lam = 0, mu = H and
 * s* = x_H (so s* = x_mu in both cases).  Cycle detection keeps O(1) state per game (Brent) with a step budget that
 * decides "found" exactly by mu + lam <= H.
 *   cycle_reward[i][g] = (sum_{j<lam} reward_i at F^j(s*), added in that order from 0.0) / lam, cycle_action the
 *   same for the scaled action; both 0 when lam = 0.
 * Deviation path y_0 = s*: for tau < L agent d plays dev_action, or with dev_action = -1 its one-period best
 * response at y_tau (the argmax over d's actions of d's env_step reward with the others greedy at y_tau, first
 * maximum under strict >); for tau >= L every agent is greedy.  act_dev[g] = d's action at tau = 0.  Rows
 * reward_rows / action_rows [row_count][N][G] hold, for tau in [row_begin, row_begin + row_count), the rewards and
 * scaled actions of the transition taken at y_tau: the layout of the episode rows, so thrl_group_stats reduces them
 * as they are (E = row_count).  The kernel walks the whole path whatever rows it stores.
 * Baseline path z_0 = s*, every agent greedy.
 * gain[g] = sum_{tau<K} w_tau * (r_d(y_tau) - r_d(z_tau)), w_0 = 1, w_{tau+1} = w_tau * gamma_d, each operation rounded
 *   once (subtract, multiply, add); gamma_d = sweep_gamma[d][g] when given, else cfg.gamma[d].
 * Return: (mu_post, lam_post) = the cycle of F from y_L under the same horizon rule; ret_step[g] = L + mu_post if that
 *   cycle is found and s* lies on it, else -1 (always -1 when lam = 0).
 * The profit gain (sum_i cycle_reward_i - Nash) / (Cartel - Nash) is the caller's (th_rl_amd/deviation.py).
 *
 * Returns THRL_ERR_BAD_CONFIG for a deviator outside [0, N), dev_len < 1, n_steps < dev_len or > THRL_DEV_MAX_STEPS,
 * horizon outside [1, THRL_DEV_MAX_HORIZON], dev_action outside {-1} + [0, n_actions[d]), a row range outside
 * [0, n_steps) or n_games outside [1, cfg.n_games]; THRL_ERR_NULL for a missing q, state0 or per-game output.
 */
#define THRL_DEV_MAX_STEPS (1 << 20)
#define THRL_DEV_MAX_HORIZON (1 << 24)
typedef struct {
    int32_t n_games;                 /* G                                                */
    int32_t deviator;                /* d in [0, N)                                      */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K >= L                                           */
    int32_t horizon;                 /* H >= 1 (th_rl_amd: min(prod_i n_actions_i + 1, 65536)) */
    int32_t dev_action;              /* fixed action index of d, or -1 = best response   */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    const double* state0;            /* device [G] start prices (required)               */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    int32_t* mu;                     /* device outputs [G]                               */
    int32_t* lam;
    int32_t* mu_post;
    int32_t* lam_post;
    int32_t* ret_step;
    int32_t* act_dev;
    double*  cycle_reward;           /* device [N][G]                                    */
    double*  cycle_action;           /* device [N][G]                                    */
    double*  gain;                   /* device [G]                                       */
    double*  reward_rows;            /* device [row_count][N][G] or NULL                 */
    double*  action_rows;            /* device [row_count][N][G] or NULL                 */
} thrl_deviation_args;
int thrl_deviation(const thrl_cfg* cfg, const void* q, const thrl_deviation_args* args, void* stream);

/*
 * Convergence tracking of the greedy policies (the stopping rule of Calvano et al., AER 2020: a session has
 * converged when no agent's greedy strategy has changed for W periods).  No reference counterpart.  QTable agents
 * only; q is read only.  Every [G] array here has G = args.n_games: the first n_games games of q.
 *
 * Policy of game g: for every agent i and every row r of its table, all n_states_i + 1 of them, the greedy action
 * argmax_row(q[g] agent i row r): the first maximum under strict > (the rule of thrl_play_greedy, thrl_deviation and
 * numpy.argmax).  policy[g] holds the P = sum_i (n_states_i + 1) entries, agent 0's rows first, one uint16 each.
 *
 * With THRL_TRACK_BASELINE: policy[g] = the policy, stable_since[g] = episode, converged_at[g] = conv_since[g] = -1,
 * changes[g] = 0; nothing is compared and nothing converges.
 * Otherwise, a check at episode e (= args.episode) does for every game g, in this order:
 *   1. if any entry of the policy differs from policy[g]: policy[g] = the policy, stable_since[g] = e, changes[g] += 1;
 *   2. if converged_at[g] < 0 and e - stable_since[g] >= W (= args.window): converged_at[g] = e,
 *      conv_since[g] = stable_since[g], *n_converged += 1 (when given), and when q_conv is given q_conv[g] = q[g]
 *      (the game's stride elements, in q's dtype) and state_conv[g] = state[g].
 * Converged games go on being tracked: stable_since and changes keep updating, converged_at keeps the first
 * convergence.  A change that reverts between two checks is not seen.
 *
 * Returns THRL_ERR_BAD_CONFIG for window < 1, n_games outside [1, cfg.n_games], a flag other than
 * THRL_TRACK_BASELINE, an agent with more than 65,536 actions, or q_conv without state or state_conv;
 * THRL_ERR_NULL for a missing q, policy, stable_since, converged_at, conv_since or changes.
 */
#define THRL_TRACK_BASELINE 1
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t flags;                   /* 0 or THRL_TRACK_BASELINE                         */
    int64_t episode;                 /* e: episodes completed so far (global index)      */
    int64_t window;                  /* W >= 1 episodes                                  */
    uint16_t* policy;                /* device [G][P] in/out                             */
    int64_t* stable_since;           /* device [G] in/out                                */
    int64_t* converged_at;           /* device [G] in/out, -1 = not (yet) converged      */
    int64_t* conv_since;             /* device [G] in/out, -1 = not (yet) converged      */
    int32_t* changes;                /* device [G] in/out: checks at which the policy changed */
    int32_t* n_converged;            /* device [1] += games that converge at this check, or NULL */
    const double* state;             /* device [G]; required with q_conv                 */
    void*    q_conv;                 /* device [G][stride] in q's dtype, or NULL         */
    double*  state_conv;             /* device [G]; required with q_conv                 */
} thrl_policy_track_args;
int thrl_policy_track(const thrl_cfg* cfg, const void* q, const thrl_policy_track_args* args, void* stream);

/*
 * Equilibrium check of the greedy strategies (Calvano et al., AER 2020, equilibrium play and "Q-loss"): hold the
 * rivals' greedy strategies fixed, solve agent i's dynamic problem exactly, and report whether its own greedy
 * strategy is a best response on the path greedy play follows (Nash) and in every state (subgame perfect), and how
 * much value it gives up if not.  No reference counterpart.  QTable agents only, no env noise (intercept env_a;
 * thrl_equilibrium_noise below is the check under noise); q, and everything else of the batch, is read only.  Every
 * [.][G] array has G = args.n_games: the first n_games games of q.  All arithmetic is float64, every operation rounded
 * once, in the order written here.
 *
 * States.  Action tuples t = (a_0 .. a_{N-1}) are numbered with agent 0 slowest, T = prod_i n_actions_i of them.
 * Tuple t gives the price p(t) (scale_action, env_step) with rewards r_i(t), and the row tuple
 * x(t) = (encode64_i(p(t)))_i.  The state set is the set of DISTINCT ROW TUPLES, numbered 0 .. S-1 in order of first
 * occurrence in tuple order; state(t) is the number of x(t), row_i(s) agent i's row in state s.  The library derives
 * these tables from cfg on the host and keeps them on the device (a few configs are cached per process).
 * Limits: T <= THRL_EQ_MAX_TUPLES and S <= THRL_EQ_MAX_STATES, otherwise THRL_ERR_UNSUPPORTED.
 *
 * Agent i's problem in game g.  pi_j(s) = argmax_row of agent j's row row_j(s) (first maximum under strict >).
 * t(s, a) = the tuple with a in place i and pi_j(s) elsewhere, R(s, a) = r_i(t(s, a)), nxt(s, a) = state(t(s, a)).
 * gamma = sweep_gamma[i][g] when given, else cfg.gamma[i].  The discounted sums below need gamma in [0, 1): without
 * sweep_gamma, cfg.gamma[i] outside it for a selected agent is THRL_ERR_BAD_CONFIG (no other analysis call
 * restricts gamma: thrl_deviation's gain is a finite sum and takes any).  The values of sweep_gamma live on the
 * device and are the caller's to check; a game whose gamma is not in [0, 1) is not solved and gets iters = -1,
 * n_diff_all = n_diff_on = 0 and NaN in every float64 output of that agent.
 *
 * Evaluation of a strategy sigma by doubling: V = R(., sigma), n = nxt(., sigma), w = gamma; D times, for all states
 * at once from the old V and n:  V = V + w * V[n];  n = n[n];  w = w * w.   D = the number of squarings w = w * w
 * (from w = gamma) until w < 2^-64: 0 for gamma = 0, 10 for 0.95, 13 for 0.99, at most 59 for any double below 1
 * (the kernel stops at 64).  The result is the discounted sum of the first 2^D rewards.
 *
 * Policy iteration from the agent's own strategy: sigma_0 = pi_i.  Round k = 0, 1, ..: V_k = evaluation of sigma_k;
 * if k == THRL_EQ_MAX_ITERS stop with iters = -1; Q(s, a) = R(s, a) + gamma * V_k[nxt(s, a)];
 * sigma_{k+1}(s) = sigma_k(s) unless max_a Q(s, a) > Q(s, sigma_k(s)), then the first maximum (strict >, a ascending);
 * if no state changed stop with iters = k.  V_pi = V_0, V* = the last V_k, sigma* = the last strategy.  The incumbent
 * is kept on ties, so a strategy that is a best response gives iters = 0 and V* == V_pi bit for bit.
 *   loss(s) = 0.0 where V*(s) == V_pi(s) or V*(s) == 0, else (V*(s) - V_pi(s)) / V*(s).
 *
 * Path.  x_0 = (encode64_i(state0[g]))_i, which need not be a member of the state set; x_{k+1} = x(tuple of the greedy
 * actions at x_k), a member.  mu >= 0, lam >= 1 the smallest values with x_{mu+lam} = x_mu: thrl_deviation's mu and lam
 * for a horizon of at least T + 1 (th_rl_amd's default).  "On path" = the lam states x_mu .. x_{mu+lam-1}, in that
 * ("cycle") order.
 *
 * Outputs, per selected agent i (bit i of agents) and game; entries of agents not selected are not written:
 *   iters, n_diff_all, n_diff_on   states / cycle states with sigma*(s) != pi_i(s)
 *   loss_all, loss_on              the largest loss(s) over all states / cycle states
 *   loss_all_mean, loss_on_mean    (sum of loss(s) from 0.0 in state order / cycle order) / S, / lam
 *   v_on                           (sum of V_pi(s) from 0.0 in cycle order) / lam
 *   br_policy, v_opt, v_pi         optional [N][G][S]: sigma*, V*, V_pi per state
 * *n_states (HOST, optional) receives S as soon as cfg is accepted, whatever the call returns afterwards.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], agents == 0 or with a bit >= N, or gamma as
 * above; THRL_ERR_UNSUPPORTED for the limits; THRL_ERR_NULL for a missing q, state0 or required output.
 */
#define THRL_EQ_MAX_ITERS 64
#define THRL_EQ_MAX_TUPLES 4096
#define THRL_EQ_MAX_STATES 1024
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t agents;                  /* bit i set: solve agent i                         */
    const double* state0;            /* device [G] start prices                          */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    int32_t* n_states;               /* HOST [1] <- S, or NULL                           */
    int32_t* mu;                     /* device [G]                                       */
    int32_t* lam;                    /* device [G]                                       */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* n_diff_all;             /* device [N][G]                                    */
    int32_t* n_diff_on;              /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_on;                /* device [N][G]                                    */
    double*  loss_all_mean;          /* device [N][G]                                    */
    double*  loss_on_mean;           /* device [N][G]                                    */
    double*  v_on;                   /* device [N][G]                                    */
    uint16_t* br_policy;             /* device [N][G][S] or NULL                         */
    double*  v_opt;                  /* device [N][G][S] or NULL                         */
    double*  v_pi;                   /* device [N][G][S] or NULL                         */
} thrl_equilibrium_args;
int thrl_equilibrium(const thrl_cfg* cfg, const void* q, const thrl_equilibrium_args* args, void* stream);

/*
 * Cross-play: greedy play between agents of DIFFERENT games (Eschenbaum, Mellgren, Zahn, "Robust algorithmic
 * collusion", 2022): seat agent 0 of one game against agent 1 of another, which never met in training, and find
 * the limit cycle of their greedy play.  No reference counterpart.  QTable agents only, no env noise (intercept
 * env_a); q, and everything else of the batch, is read only.
 *
 * G = args.n_games: the first n_games games of q (1 <= G <= cfg.n_games).  M = args.n_matches >= 1 matches; every
 * [.][M] array here is indexed by match.  seat (device int32 [N][M]): in match m, seat i is taken by AGENT i OF GAME
 * seat[i][m].  Roles are kept -- agents may have different grids, so seat i always plays from an agent-i table.
 * Identity seats (M = G, seat[i][m] = m) give thrl_deviation's pre-shock cycle of every game.
 *
 * Greedy map F of match m on row tuples x = (row_0 .. row_{N-1}): a_i = argmax_row of row x_i of agent i's table in
 * q[seat[i][m]] (first maximum under strict >), then exactly thrl_deviation's F: scale_action and env_step with NO
 * env noise give the price p and the rewards, F(x)_i = encode64_i(p).  The reward and scaled action "at x" are those
 * of the transition taken at x.
 *
 * Start state x_0 = (encode64_i(state0[m]))_i.  (mu, lam), s*, cycle_reward and cycle_action are thrl_deviation's,
 * word for word: mu >= 0, lam >= 1 the smallest values with x_{mu+lam} = x_mu; the cycle is found iff
 * mu + lam <= H (horizon), then s* = x_mu; otherwise lam = 0 and mu = H.  Cycle detection keeps O(1) state per match
 * (Brent) with a step budget that decides "found" exactly by mu + lam <= H.
 *   cycle_reward[i][m] = (sum_{j<lam} reward_i at F^j(s*), added in that order from 0.0) / lam, cycle_action the same
 *   for the scaled action; both 0 when lam = 0.
 * Rows reward_rows / action_rows [row_count][N][M] (each optional) hold, for tau in [row_begin, row_begin + row_count)
 * inside [0, n_steps), the rewards and scaled actions of the transition taken at x_tau -- the path from x_0, before
 * and on the cycle: the layout of the episode rows, so thrl_group_stats reduces them as they are (E = row_count,
 * G = M).  All arithmetic is float64, every operation rounded once, in thrl_deviation's order.
 *
 * policy (device uint16 [G][P], P = sum_i (n_states_i + 1), the layout of thrl_policy_track): the matches are played
 * from the greedy policies, not from q.  Without THRL_XPLAY_POLICY_GIVEN the call first fills policy[g] for every
 * g < G from q (one streaming pass; the array thrl_policy_track writes with THRL_TRACK_BASELINE) and then plays;
 * with the flag it plays from what policy holds and q may be NULL.  So a caller extracts once and plays any number
 * of re-pairings, and the policy array of a convergence tracker can be played as it is.  Entries that are no action
 * of their agent are the caller's to avoid (they are clamped to the last action, nothing is read out of bounds).
 *
 * A seat outside [0, G) is device data the host cannot see: that match reads nothing and gets mu = -1, lam = 0 and
 * zeros in cycle_reward, cycle_action and its rows.  No other match is affected.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_matches < 1, n_games outside [1, cfg.n_games], horizon outside
 * [1, THRL_DEV_MAX_HORIZON], n_steps outside [0, THRL_DEV_MAX_STEPS], a row range outside [0, n_steps), a flag other
 * than THRL_XPLAY_POLICY_GIVEN or an agent with more than 65,536 actions; THRL_ERR_NULL for a missing seat, state0,
 * policy, mu, lam, cycle_reward or cycle_action, or a missing q without THRL_XPLAY_POLICY_GIVEN.
 */
#define THRL_XPLAY_POLICY_GIVEN 1
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]: games of q / policy       */
    int32_t n_matches;               /* M >= 1                                           */
    int32_t n_steps;                 /* K in [0, THRL_DEV_MAX_STEPS]: length of the path the rows are cut from */
    int32_t horizon;                 /* H >= 1 (th_rl_amd: min(prod_i n_actions_i + 1, 65536)) */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t flags;                   /* 0 or THRL_XPLAY_POLICY_GIVEN                     */
    int32_t reserved;                /* 0                                                */
    const int32_t* seat;             /* device [N][M]: game whose agent i sits in match m */
    const double* state0;            /* device [M] start prices                          */
    uint16_t* policy;                /* device [G][P]: out without the flag, in with it  */
    int32_t* mu;                     /* device outputs [M]                               */
    int32_t* lam;
    double*  cycle_reward;           /* device [N][M]                                    */
    double*  cycle_action;           /* device [N][M]                                    */
    double*  reward_rows;            /* device [row_count][N][M] or NULL                 */
    double*  action_rows;            /* device [row_count][N][M] or NULL                 */
} thrl_crossplay_args;
int thrl_crossplay(const thrl_cfg* cfg, const void* q, const thrl_crossplay_args* args, void* stream);

/*
 * Attractor analysis of the greedy strategies: ALL limit cycles of a game's greedy play and their basins, not only the
 * one the training state falls into (thrl_deviation, thrl_equilibrium and thrl_crossplay follow one path).  No
 * reference counterpart: utils.play_game starts every evaluation from environment.reset(), a uniform draw on [0, a),
 * and plot_mean_conf / plot_sweep_conf average over such draws; reset_reward below is the exact value of that
 * expectation for greedy play.  QTable agents only, no env noise (intercept env_a); q, and everything else of the
 * batch, is read only.  Every [.][G] array has G = args.n_games: the first n_games games of q.  All arithmetic is
 * float64, every operation rounded once, in the order written here.
 *
 * States.  Exactly thrl_equilibrium's: action tuples t (agent 0 slowest, T of them), rewards r_i(t), the scaled action
 * sc_i(t) = scale_action of agent i's action in t, state(t), and the S distinct row tuples numbered by first
 * occurrence in tuple order with rows row_i(s); the same limits (THRL_EQ_MAX_TUPLES, THRL_EQ_MAX_STATES, otherwise
 * THRL_ERR_UNSUPPORTED) and the same cached per-config plan.  A game's working set lives in one block's LDS; a config
 * inside the limits that needs more than 64 KB of it (six or more agents with S near the limit) is
 * THRL_ERR_UNSUPPORTED too.
 *
 * Policies.  policy (device uint16 [G][P], P = sum_i (n_states_i + 1), the layout of thrl_policy_track): without
 * THRL_ATTR_POLICY_GIVEN the call first fills policy[g] for every g < G from q (thrl_crossplay's extraction pass) and
 * then works from it; with the flag it works from what policy holds and q may be NULL.  So one extraction, or the
 * policy array of a convergence tracker, serves this call and cross-play alike.  Entries that are no action of their
 * agent are clamped to the last action (nothing is read out of bounds).
 *
 * Map.  pi_i(r) = the policy entry of agent i's row r.  t(s) = the tuple (pi_i(row_i(s)))_i, f(s) = state(t(s)).  For
 * every state s: mu(s) = the smallest k >= 0 for which f^k(s) lies on a cycle of f, rep(s) = the smallest state number
 * on that cycle, lam(s) = its length.
 *
 * Attractors of a game = the distinct values of rep, n_attr of them.  basin(r) = the number of states s with
 * rep(s) = r, the cycle's own states included.  Order: basin descending, ties by rep ascending.  The first
 * THRL_ATTR_KEEP are reported, slot k of game g at [k][G] / [k][N][G]:
 *   rep, lam, basin
 *   cycle_reward[k][i][g] = (sum_{j<lam} r_i(t(f^j(rep))), added in that order from 0.0) / lam
 *   cycle_action[k][i][g] = the same for sc_i
 * Slots k >= n_attr get rep = -1, lam = 0, basin = 0 and zeros.  Per game: n_attr, mu_max = max_s mu(s),
 * n_cycle_states = the sum of lam over all attractors, kept or not.
 *
 * Training state.  x_0 = (encode64_i(state0[g]))_i, which need not be a member of the state set; its successor
 * state(tuple of the greedy actions at x_0's rows) is.  rep_x0 = rep of the cycle x_0 reaches, mu_x0 = the steps to
 * it -- thrl_deviation's mu for a horizon of at least T + 1, and lam of rep_x0's attractor is its lam -- and
 * slot_x0 = that attractor's slot, or -1 if it is not among the kept.
 *
 * Reset distribution (optional: n_starts = 0 skips it, its tables and outputs may then be NULL).  The caller cuts
 * [0, env_a) at every agent's encode breakpoints into J = n_starts intervals: start_rows (device int32 [N][J]) holds
 * agent i's row on interval j, start_w (device double [J]) its length / env_a (th_rl_amd.attractors.starts).  Rows
 * are clamped to [0, n_states_i].  Start j reaches the attractor A(j) of state(tuple of pi_i(start_rows[i][j])).
 *   reset_mass[k][g]    = sum of w_j over the j with A(j) in slot k, reset_mass_other[g] over the j whose attractor
 *                         is not kept; both added in ascending j from 0.0
 *   reset_reward[i][g]  = sum_j w_j * cycle_reward_i(A(j)) over ALL j, kept or not, in ascending j from 0.0, each
 *                         multiply and each add rounded once
 *
 * state_rep, state_mu (optional, uint16 [G][S]): rep(s) and mu(s) of every state.
 * *n_states (HOST, optional) receives S as soon as cfg is accepted, whatever the call returns afterwards.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], a flag other than THRL_ATTR_POLICY_GIVEN or
 * n_starts outside [0, THRL_ATTR_MAX_STARTS]; THRL_ERR_UNSUPPORTED for the limits; THRL_ERR_NULL for a missing
 * state0, policy or per-game / per-slot output, a missing q without THRL_ATTR_POLICY_GIVEN, or with n_starts > 0 a
 * missing start_rows, start_w, reset_mass, reset_mass_other or reset_reward.
 */
#define THRL_ATTR_KEEP 8
#define THRL_ATTR_POLICY_GIVEN 1
#define THRL_ATTR_MAX_STARTS (1 << 20)
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t flags;                   /* 0 or THRL_ATTR_POLICY_GIVEN                      */
    int32_t n_starts;                /* J in [0, THRL_ATTR_MAX_STARTS]                   */
    int32_t reserved;                /* 0                                                */
    const double* state0;            /* device [G] training states (prices)              */
    uint16_t* policy;                /* device [G][P]: out without the flag, in with it  */
    const int32_t* start_rows;       /* device [N][J], or NULL with J = 0                */
    const double* start_w;           /* device [J], or NULL with J = 0                   */
    int32_t* n_states;               /* HOST [1] <- S, or NULL                           */
    int32_t* n_attr;                 /* device [G]                                       */
    int32_t* mu_max;                 /* device [G]                                       */
    int32_t* n_cycle_states;         /* device [G]                                       */
    int32_t* rep;                    /* device [KEEP][G]                                 */
    int32_t* lam;                    /* device [KEEP][G]                                 */
    int32_t* basin;                  /* device [KEEP][G]                                 */
    double*  cycle_reward;           /* device [KEEP][N][G]                              */
    double*  cycle_action;           /* device [KEEP][N][G]                              */
    int32_t* rep_x0;                 /* device [G]                                       */
    int32_t* mu_x0;                  /* device [G]                                       */
    int32_t* slot_x0;                /* device [G]                                       */
    double*  reset_mass;             /* device [KEEP][G], or NULL with J = 0             */
    double*  reset_mass_other;       /* device [G], or NULL with J = 0                   */
    double*  reset_reward;           /* device [N][G], or NULL with J = 0                */
    uint16_t* state_rep;             /* device [G][S] or NULL                            */
    uint16_t* state_mu;              /* device [G][S] or NULL                            */
} thrl_attractors_args;
int thrl_attractors(const thrl_cfg* cfg, const void* q, const thrl_attractors_args* args, void* stream);

/*
 * Greedy play under demand noise: the exact long-run behaviour of a game's greedy strategies in the environment the
 * reference ships, NoisyPriceState with noise_prob > 0, which redraws the demand intercept from U(0.7 a, a) with that
 * probability at every step (utils.play_game, behind plot_mean_conf / plot_sweep_conf / plot_mean_result, steps through
 * it).  thrl_deviation, thrl_equilibrium, thrl_crossplay and thrl_attractors describe the deterministic greedy map;
 * that map usually has several limit cycles, and a demand shock moves a game from one to another, so the profit that
 * greedy play sustains belongs to no single cycle: it is the stationary behaviour of a Markov chain.  With the price
 * axis cut at the agents' encode breakpoints the chain is finite, and this call iterates it; the only other route,
 * thrl_play_greedy with noise, samples it.  QTable agents only; q, and everything else of the batch, is read only.
 * Every [.][G] array has G = args.n_games: the first n_games games of q.  All arithmetic is float64, every operation
 * rounded once, in the order written here.
 *
 * Cells.  The caller cuts [0, env_a) at every agent's encode breakpoints into J = n_cells cells [c_k, c_{k+1})
 * (th_rl_amd.attractors.starts): cell_rows (device int32 [N][J]) holds agent i's row on cell k (clamped to
 * [0, n_states_i]), cell_w (device double [J]) the cell's length / env_a.  A noise-free price that sits exactly on a
 * breakpoint where the agents' half-even ties disagree has a row tuple that no interval has; the caller appends every
 * such row tuple as a POINT CELL (its rows, cell_w = 0, no band entry: a redrawn intercept lands on a single price with
 * probability 0), so the cells are any J distinct row tuples with weights.  J <= THRL_STAT_MAX_CELLS, above it
 * THRL_ERR_UNSUPPORTED; the same when a game's working set (two iterates and the tuple per cell, 18 J bytes, plus
 * 512 (2 N + 2) bytes of staging) does not fit one block's 64 KB of LDS.
 *
 * Tuples.  thrl_equilibrium's: action tuples t (agent 0 slowest, T of them), the noise-free price p(t) and rewards
 * r_i(t) (scale_action, env_step with intercept env_a), the scaled action sc_i(t); the limit THRL_EQ_MAX_TUPLES and
 * the same cached per-config plan.  *n_tuples (HOST, optional) receives T as soon as cfg is accepted.
 *
 * Per-config tables, computed by the caller (th_rl_amd.stationary.tables) and only read here, so that the device and
 * a host restatement share their bits.  With u(t) = the amount env_step subtracts from the intercept (env_b * Q),
 * noise_lo = 0.7 env_a, lo = noise_lo - u, hi = env_a - u, width = env_a - noise_lo:
 *   det_cell (device int32 [T])      the cell whose row tuple equals (encode64_i(p(t)))_i: the noise-free part of the
 *                                    chain is thrl_deviation's F.  An entry outside [0, J) is no cell: that mass is lost
 *   band_lo (device int32 [T]), band (device double [T][W], W = band_w)
 *                                    n(t, k) = band[t][k - band_lo[t]] where 0 <= k - band_lo[t] < W, else 0: the
 *                                    probability that a redrawn intercept puts the price of t into cell k,
 *                                    (len_k + [k = 0] z) / width with len_k = max(0, min(c_{k+1}, hi) - max(c_k, lo))
 *                                    and z = max(0, -lo) - max(0, -hi), the mass of prices clipped to 0
 *   noise_price (device double [T])  the expected price of t under a redrawn intercept: (lo + hi) / 2 if lo >= 0,
 *                                    0 if hi <= 0, else hi^2 / (2 width)
 *   noise_reward (device double [N][T])  that price times agent i's quantity in t (env_step's ratio * sc_i)
 *
 * Noise probability.  p_g = args.noise_prob, or noise_prob_g[g] where that array (device double [G]) is given, then
 * args.noise_prob is not read; q_g = 1 - p_g.  It need not be the one the games were trained with.  A host-visible
 * value outside (0, 1] is THRL_ERR_BAD_CONFIG; an entry of noise_prob_g outside it (NaN included) is device data: that
 * game gets iters = -1 and zeros in every output, and no other game is affected.
 *
 * Policies.  policy (device uint16 [G][P], P = sum_i (n_states_i + 1), the layout of thrl_policy_track): without
 * THRL_STAT_POLICY_GIVEN the call first fills policy[g] for every g < G from q (thrl_crossplay's extraction pass) and
 * then works from it; with the flag it works from what policy holds and q may be NULL.  Entries that are no action of
 * their agent are clamped to the last action (nothing is read out of bounds).  t_g(k) = the tuple of the policy
 * entries at cell_rows[.][k].
 *
 * Chain.  P_g(j, k) = q_g [det_cell(t_g(j)) = k] + p_g n(t_g(j), k): the product p_g * n is computed, and q_g is added
 * to it only where the bracket is 1.
 *
 * Iteration, in the lazy form (I + P) / 2, which converges for every finite chain to the Cesaro limit from the start
 * distribution whatever the periods (a chain with p = 1 whose band alternates between two cells has no other limit).
 *   mu_0 = cell_w (the environment's reset distribution), or with THRL_STAT_START_STATE the unit mass on the cell
 *          whose row tuple equals (encode64_i(state0[g]))_i; a game whose state0 has the rows of no cell (a price on a
 *          breakpoint where the ties disagree, which is no noise-free price) gets iters = -1 and zeros
 *   s(k) = sum_j mu_m(j) * P_g(j, k), in ascending j from 0.0 (terms that are zero may be skipped: adding +0.0 is
 *          exact)
 *   mu_{m+1}(k) = 0.5 * mu_m(k) + 0.5 * s(k)
 *   chg_m = max_k |mu_{m+1}(k) - mu_m(k)|
 * Stop after the first step with chg <= args.tol, or after args.max_iters steps.
 *
 * Outputs, per game, from the last iterate mu; every sum over ascending k from 0.0, each multiply and add rounded once:
 *   iters                the steps taken (= max_iters: the tolerance was not reached), change = the last chg
 *   mass                 sum_k mu(k)
 *   stat_reward[i][g]    sum_k mu(k) * (q_g * r_i(t(k)) + p_g * noise_reward_i(t(k)))
 *   stat_action[i][g]    sum_k mu(k) * sc_i(t(k))
 *   stat_price[g]        sum_k mu(k) * (q_g * p(t(k)) + p_g * noise_price(t(k)))
 *   pi (optional, double [G][J])   mu itself
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], an unknown flag, n_cells < 1, band_w < 1,
 * max_iters outside [1, THRL_STAT_MAX_ITERS], tol < 0 or NaN, or noise_prob as above; THRL_ERR_UNSUPPORTED for the
 * limits; THRL_ERR_NULL for a missing table (cell_rows, cell_w, det_cell, band_lo, band, noise_reward, noise_price),
 * policy or per-game output, a missing state0 with THRL_STAT_START_STATE, or a missing q without
 * THRL_STAT_POLICY_GIVEN.
 */
#define THRL_STAT_POLICY_GIVEN 1
#define THRL_STAT_START_STATE 2
#define THRL_STAT_MAX_CELLS 4096
#define THRL_STAT_MAX_ITERS 65536
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t flags;                   /* THRL_STAT_POLICY_GIVEN | THRL_STAT_START_STATE   */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t max_iters;               /* in [1, THRL_STAT_MAX_ITERS]                      */
    int32_t reserved;                /* 0                                                */
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  tol;                     /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const double* state0;            /* device [G] prices, with THRL_STAT_START_STATE    */
    uint16_t* policy;                /* device [G][P]: out without the flag, in with it  */
    const int32_t* cell_rows;        /* device [N][J]                                    */
    const double* cell_w;            /* device [J]                                       */
    const int32_t* det_cell;         /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* noise_price;       /* device [T]                                       */
    int32_t* n_tuples;               /* HOST [1] <- T, or NULL                           */
    int32_t* iters;                  /* device [G]                                       */
    double*  change;                 /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  stat_reward;            /* device [N][G]                                    */
    double*  stat_action;            /* device [N][G]                                    */
    double*  stat_price;             /* device [G]                                       */
    double*  pi;                     /* device [G][J] or NULL                            */
} thrl_stationary_args;
int thrl_stationary(const thrl_cfg* cfg, const void* q, const thrl_stationary_args* args, void* stream);

/*
 * Equilibrium check under demand noise: thrl_equilibrium's question -- is agent i's greedy strategy a best response to
 * the rivals' greedy strategies, and which share of the attainable value does it give up if not -- in the environment
 * of thrl_stationary, where the demand intercept is redrawn with probability p at every step.  Under noise a game does
 * not follow one path into one cycle: every price cell is reachable, the continuation value of an action is an
 * expectation over where a shock puts the price, and a strategy's value solves a linear system on the cells.  There is
 * no path, so there are no on-path outputs; the long-run distribution over the cells (thrl_stationary's pi) may be handed
 * in as weights.  No reference counterpart.  QTable agents only; q, and everything else of the batch, is read only.
 * Every [.][G] array has G = args.n_games: the first n_games games of q.  All arithmetic is float64, every operation
 * rounded once, in the order written here.
 *
 * Cells, tuples, per-config tables, noise probability, policies: thrl_stationary's, word for word (cell_rows, det_cell,
 * band_lo, band, noise_reward with J = n_cells and W = band_w; r_i(t) from the cached per-config plan; p_g and q_g = 1 -
 * p_g; policy with or without THRL_EQN_POLICY_GIVEN; t_g(k) = the tuple of the clamped policy entries at
 * cell_rows[.][k]).  cell_w and noise_price are not read.  *n_tuples (HOST, optional) receives T as soon as cfg is
 * accepted.
 *
 * Agent i's problem in game g, with p = p_g, q = q_g, gamma = sweep_gamma[i][g] when given, else cfg.gamma[i] (the
 * rules of thrl_equilibrium: without sweep_gamma a cfg.gamma[i] outside [0, 1) of a selected agent is
 * THRL_ERR_BAD_CONFIG).  pi_i(k) = agent i's action in t_g(k); t(k, a) = t_g(k) with a in place i.
 *   R(k, a) = q * r_i(t) + p * noise_reward_i(t)  with t = t(k, a)  (thrl_stationary's expected reward)
 *   z_V(t)  = q * V[det_cell(t)] + p * b,  b = the sum over w = 0 .. W-1, ascending, from 0.0, of
 *             band[t][w] * V[band_lo[t] + w]; terms whose cell band_lo[t] + w lies outside [0, J) are skipped, and the
 *             q term is +0.0 where det_cell(t) lies outside [0, J) (it is still added).  z depends on the tuple alone.
 *
 * Evaluation of a strategy sigma from a start V^0 (Jacobi, all cells from the old iterate):
 *   V^{m+1}(k) = R(k, sigma(k)) + gamma * z_{V^m}(t(k, sigma(k)))
 *   chg_m = max_k |V^{m+1}(k) - V^m(k)|
 * Stop after the first sweep with chg <= eval_tol.  An evaluation that has made max_sweeps sweeps without that is
 * CAPPED.  The iterates contract with factor gamma in the maximum norm, so a stopped evaluation is within
 * gamma / (1 - gamma) * eval_tol of the strategy's true value.
 *
 * Policy iteration from the agent's own strategy: sigma_0 = pi_i, V^0 = 0 in round 0, the previous round's V after it.
 * Round n = 0, 1, ..: V_n = evaluation of sigma_n; if n == THRL_EQ_MAX_ITERS the (agent, game) is capped;
 *   Q(k, a) = R(k, a) + gamma * z_{V_n}(t(k, a))
 *   margin = ((2 * gamma) * gamma) * eval_tol / (1 - gamma)    (three products left to right, then one division)
 *   sigma_{n+1}(k) = sigma_n(k) unless max_a Q(k, a) > Q(k, sigma_n(k)) + margin, then the first maximum (strict >, a
 *   ascending); if no cell changed stop with iters = n.
 * Why the margin: both Q(k, a) and Q(k, sigma_n(k)) carry gamma times the evaluation's error, at most gamma^2 / (1 -
 * gamma) * eval_tol each, so a difference above 2 gamma^2 / (1 - gamma) * eval_tol is an improvement of the true values
 * and the iteration cannot cycle on evaluation error.  With eval_tol = 0 the margin is 0 and the rule is
 * thrl_equilibrium's keep-the-incumbent rule.  V_pi = V_0, V* = the last V_n, sigma* = the last strategy,
 *   loss(k) = 0.0 where V*(k) == V_pi(k) or V*(k) == 0, else (V*(k) - V_pi(k)) / V*(k).
 *
 * Outputs, per selected agent i (bit i of agents) and game; entries of agents not selected are not written:
 *   iters            the rounds n (0: pi_i is a best response in every cell), -1 when not solved
 *   sweeps           all evaluation sweeps of the (agent, game)
 *   n_diff_all       cells with sigma*(k) != pi_i(k)
 *   loss_all         the largest loss(k);  loss_all_mean = (sum of loss(k) over ascending k from 0.0) / J
 *   with weights (device double [G][J], e.g. thrl_stationary's pi; NULL: the three outputs are not written), each a sum
 *   over ascending k from 0.0:
 *     loss_w = sum w(k) * loss(k),  diff_w = sum of w(k) over the cells with sigma*(k) != pi_i(k) (+0.0 elsewhere),
 *     v_w = sum w(k) * V_pi(k)
 *   br_policy, v_opt, v_pi   optional [N][G][J]: sigma*, V*, V_pi per cell
 *
 * Games that are not solved; no other game is affected.  An entry of noise_prob_g outside (0, 1] (NaN included):
 * iters = -1 and zeros in every output of every selected agent, the optional ones included (thrl_stationary's rule).
 * Otherwise a gamma outside [0, 1) (NaN included), or a capped (agent, game): iters = -1, n_diff_all = 0, sweeps = the
 * sweeps made, NaN in every float64 output of that agent, and br_policy = pi_i (thrl_equilibrium's rule).
 *
 * Limits: T <= THRL_EQ_MAX_TUPLES, J <= THRL_STAT_MAX_CELLS and a game's working set in one block's 64 KB of LDS:
 * 50 J + 2064 bytes (three value arrays, the strategy, its reward, successor and band place per cell, the tuples, and
 * 2,048 bytes of staging); otherwise THRL_ERR_UNSUPPORTED.  J = 1,269 fits.  Where 8 T more bytes fit, z is staged per
 * tuple.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], agents == 0 or with a bit >= N, a flag other than
 * THRL_EQN_POLICY_GIVEN, gamma as above, n_cells < 1, band_w < 1, max_sweeps outside [1, THRL_STAT_MAX_ITERS],
 * eval_tol < 0 or NaN, or a host-visible noise_prob outside (0, 1]; THRL_ERR_UNSUPPORTED for the limits; THRL_ERR_NULL
 * for a missing table (cell_rows, det_cell, band_lo, band, noise_reward), policy, iters, sweeps, n_diff_all, loss_all or
 * loss_all_mean, with weights a missing loss_w, diff_w or v_w, or a missing q without THRL_EQN_POLICY_GIVEN.
 */
#define THRL_EQN_POLICY_GIVEN 1
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t agents;                  /* bit i set: solve agent i                         */
    int32_t flags;                   /* 0 or THRL_EQN_POLICY_GIVEN                       */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t max_sweeps;              /* in [1, THRL_STAT_MAX_ITERS], per evaluation      */
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  eval_tol;                /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    uint16_t* policy;                /* device [G][P]: out without the flag, in with it  */
    const int32_t* cell_rows;        /* device [N][J]                                    */
    const int32_t* det_cell;         /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* weights;           /* device [G][J] or NULL                            */
    int32_t* n_tuples;               /* HOST [1] <- T, or NULL                           */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* sweeps;                 /* device [N][G]                                    */
    int32_t* n_diff_all;             /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_all_mean;          /* device [N][G]                                    */
    double*  loss_w;                 /* device [N][G], with weights                      */
    double*  diff_w;                 /* device [N][G], with weights                      */
    double*  v_w;                    /* device [N][G], with weights                      */
    uint16_t* br_policy;             /* device [N][G][J] or NULL                         */
    double*  v_opt;                  /* device [N][G][J] or NULL                         */
    double*  v_pi;                   /* device [N][G][J] or NULL                         */
} thrl_equilibrium_noise_args;
int thrl_equilibrium_noise(const thrl_cfg* cfg, const void* q, const thrl_equilibrium_noise_args* args, void* stream);

/*
 * Deviation test under demand noise: thrl_deviation's question -- does a deviation pay, do the others punish, does
 * play return -- in the environment of thrl_stationary, where the demand intercept is redrawn with probability p at
 * every step.  Under noise a game follows no single path into one cycle, so a punishment seen on one path says little
 * about what a deviator can expect; the exact answer is the propagation of a distribution: noisy greedy play is a
 * finite Markov chain on the price cells, a forced deviation replaces the deviator's action in every cell for L
 * periods, and the response is the sequence of distributions that follow from the one the shock hits.  No sampling.
 * No reference counterpart.  QTable agents only; q, and everything else of the batch, is read only.  Every [.][G]
 * array has G = args.n_games: the first n_games games of q.  All arithmetic is float64, every operation rounded once,
 * in the order written here; every sum over cells runs over ascending k (or j) from 0.0.
 *
 * Cells, tuples, per-config tables, noise probability, policies: thrl_stationary's, word for word (cell_rows, det_cell,
 * band_lo, band, noise_reward with J = n_cells and W = band_w; r_i(t) from the cached per-config plan and sc_i(t); p_g
 * and q_g = 1 - p_g; policy with or without THRL_STAT_POLICY_GIVEN, the only flag; t_g(k) = the tuple of the clamped
 * policy entries at cell_rows[.][k]).  cell_w and noise_price are not read.  *n_tuples (HOST, optional) receives T as
 * soon as cfg is accepted.
 *
 *   R_i(t)    = q_g * r_i(t) + p_g * noise_reward_i(t)   (thrl_stationary's expected reward)
 *   t'_g(k)   = t_g(k) with the deviator d's action replaced: by dev_action, or with dev_action = -1 by d's one-period
 *               best response in that cell, the argmax over d's actions a of R_d(t_g(k) with a in place d), the first
 *               maximum under strict >
 *   P_g(j, k) = q_g [det_cell(t(j)) = k] + p_g n(t(j), k), as in thrl_stationary (the product p_g * n is computed, and
 *               q_g is added to it only where the bracket is 1); P'_g the same with t'
 *   m_0       = weights[g] (device double [G][J], required): the distribution the shock hits, e.g. thrl_stationary's pi
 *   m_{tau+1}(k) = sum_j m_tau(j) * P^(tau)(j, k), P^(tau) = P' for tau < L and P otherwise, t^(tau) likewise: the plain
 *               step, not the lazy one, so the iterate after tau steps is the distribution at period tau.  Terms that
 *               are zero may be skipped: adding +0.0 is exact
 *   E_i(tau)  = sum_k m_tau(k) * R_i(t^(tau)(k)),  A_i(tau) = sum_k m_tau(k) * sc_i(t^(tau)(k))
 *   D(tau)    = 0.5 * sum_k |m_tau(k) - m_0(k)|: the total-variation distance from the start (D(0) = 0)
 *
 * Rows reward_rows / action_rows [row_count][N][G] (optional) hold E_i(tau) / A_i(tau) for tau in [row_begin, row_begin +
 * row_count): the layout of the episode rows, so thrl_group_stats reduces them as they are (E = row_count); dist_rows
 * [row_count][G] (optional) holds D(tau).  The kernel walks all K periods whatever rows it stores.
 *
 * Outputs, per game:
 *   base_reward[i][g] = sum_k m_0(k) * R_i(t(k)): the expression of thrl_stationary's stat_reward, bit-equal to it with
 *                       its pi as weights;  base_action[i][g] = sum_k m_0(k) * sc_i(t(k))
 *   dev_share[g]      = the sum of m_0(k) over the cells with t'(k) != t(k) (+0.0 elsewhere): the long-run share of
 *                       periods in which the deviation changes anything
 *   gain[g]           = sum_{tau<K} w_tau * (E_d(tau) - base_reward_d), w_0 = 1, w_{tau+1} = w_tau * gamma_d (subtract,
 *                       multiply, add); gamma_d = sweep_gamma[d][g] when given, else cfg.gamma[d]
 *   gain_dev[g]       = the same sum over tau < L: what the deviation itself earns; gain - gain_dev is the aftermath
 *   low[g]            = min_{L <= tau < K} (E_d(tau) - base_reward_d), low_step[g] its first tau; K == L: 0.0 and -1
 *   ret_step[g]       = the first tau in [L, K] with D(tau) <= ret_tol, else -1
 *   dist[g] = D(K),  mass[g] = sum_k m_K(k)
 * A game whose noise_prob_g entry lies outside (0, 1] (NaN included) gets zeros in every float64 output, its rows
 * included, and -1 in low_step and ret_step; no other game is affected (thrl_stationary's rule).
 *
 * Limits: T <= THRL_EQ_MAX_TUPLES, J <= THRL_STAT_MAX_CELLS and a game's working set in one block's 64 KB of LDS: both
 * iterates, t(k) and t'(k), and the staging of the ordered sums, 20 J + 512 (2 N + 2) + 16 bytes; otherwise
 * THRL_ERR_UNSUPPORTED.  J = 3,001 with N = 2 fits.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], an unknown flag, a deviator outside [0, N),
 * dev_len < 1, n_steps < dev_len or > THRL_DEV_MAX_STEPS, dev_action outside {-1} + [0, n_actions[d]), a row range
 * outside [0, n_steps), n_cells < 1, band_w < 1, ret_tol < 0 or NaN, or a host-visible noise_prob outside (0, 1];
 * THRL_ERR_UNSUPPORTED for the limits; THRL_ERR_NULL for a missing table (cell_rows, det_cell, band_lo, band,
 * noise_reward), weights, policy or per-game output, or a missing q without THRL_STAT_POLICY_GIVEN.  All of these are
 * decided before any launch.
 */
typedef struct {
    int32_t n_games;                 /* G in [1, cfg.n_games]                            */
    int32_t flags;                   /* 0 or THRL_STAT_POLICY_GIVEN                      */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t deviator;                /* d in [0, N)                                      */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K >= L                                           */
    int32_t dev_action;              /* fixed action index of d, or -1 = best response   */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  ret_tol;                 /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    uint16_t* policy;                /* device [G][P]: out without the flag, in with it  */
    const int32_t* cell_rows;        /* device [N][J]                                    */
    const int32_t* det_cell;         /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* weights;           /* device [G][J] (required): m_0                    */
    int32_t* n_tuples;               /* HOST [1] <- T, or NULL                           */
    double*  base_reward;            /* device [N][G]                                    */
    double*  base_action;            /* device [N][G]                                    */
    double*  dev_share;              /* device [G]                                       */
    double*  gain;                   /* device [G]                                       */
    double*  gain_dev;               /* device [G]                                       */
    double*  low;                    /* device [G]                                       */
    int32_t* low_step;               /* device [G]                                       */
    int32_t* ret_step;               /* device [G]                                       */
    double*  dist;                   /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  reward_rows;            /* device [row_count][N][G] or NULL                 */
    double*  action_rows;            /* device [row_count][N][G] or NULL                 */
    double*  dist_rows;              /* device [row_count][G] or NULL                    */
} thrl_deviation_noise_args;
int thrl_deviation_noise(const thrl_cfg* cfg, const void* q, const thrl_deviation_noise_args* args, void* stream);

/*
 * Strategies as tables over the game's action tuples, for ANY discrete agent: QTable, Reinforce, ActorCritic.  No
 * reference counterpart.  The analyses above index a policy by the agent's table row, which a network does not have.
 * The game has a finite state set of its own: with discrete agents and no env noise the price after a step is a
 * function of that step's action tuple, so what an agent does next is a function of the tuple index.  Tuples are
 * numbered with agent 0 slowest: t = sum_i k_i * prod_{j > i} n_actions_j, T = prod_i n_actions_i <=
 * THRL_TP_MAX_TUPLES.  price (device float64 [T]) holds the noise-free price after every tuple; the CALLER computes
 * it (th_rl_amd.tuple_play.tables: scale, env_step with intercept env_a, every operation rounded once, QTable agents
 * scaled by k / (A - 1), Reinforce / ActorCritic agents by k / A), the device does no scaling arithmetic.
 *
 * thrl_tuple_policy fills tuple_policy (device uint16 [G][N][T], G = args.n_games, 1 <= G <= cfg.n_games):
 * entry [g][i][t] is what get_action of agent i of game g returns at the state price[t].
 *   kind[i] = 0, QTable: the first maximum (strict >) of row encode64_i(price[t]) of agent i's table in q[g]: the
 *     entry thrl_crossplay's extraction writes for that row.
 *   kind[i] = 1 / 2, Reinforce / ActorCritic: argmax pi at x = (float)price[t], evaluated by the function
 *     thrl_nn_act / thrl_ac_act evaluate: bit for bit the action they return with u = NULL at that price.
 *     nn_params[i] (device [G][thrl_nn_param_count / thrl_ac_param_count]) as in thrl_mixed; cfg.n_actions[i] in
 *     [2, 32], cfg.n_states[i] is not read.
 * kind and nn_params have thrl_mixed's meanings; q may be NULL when no agent is a QTable.  Everything but
 * tuple_policy is read only.
 *
 * Returns THRL_ERR_UNSUPPORTED for a CAC agent (kind 3: its action is continuous) or n_tuples > THRL_TP_MAX_TUPLES;
 * THRL_ERR_BAD_CONFIG for n_games outside [1, cfg.n_games], a kind outside [0, 3], a neural agent with actions
 * outside [2, 32], n_tuples < 1 or n_tuples != prod_i n_actions_i; THRL_ERR_NULL for a missing cfg, args, price,
 * tuple_policy, nn_params[i] of a neural agent, or q with a QTable agent in the game.
 */
#define THRL_TP_MAX_TUPLES 4096
typedef struct {
    int32_t n_games;                     /* G in [1, cfg.n_games]                            */
    int32_t n_tuples;                    /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t kind[THRL_MAXA];             /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    const float* nn_params[THRL_MAXA];   /* device [G][P] for the neural agents              */
    const double* price;                 /* device [T]                                       */
    uint16_t* tuple_policy;              /* device [G][N][T], out                            */
} thrl_tuple_policy_args;
int thrl_tuple_policy(const thrl_cfg* cfg, const void* q, const thrl_tuple_policy_args* args, void* stream);

/*
 * Greedy play on tuple indices between any agents of any games, from a tuple_policy array: thrl_crossplay for
 * strategies in tuple form, with no encode and no network in it.  Of a valid cfg only n_agents and n_actions are used.
 *
 * G = args.n_games >= 1: the games of tuple_policy (it need not be cfg.n_games: the array may hold the games of
 * several batches of one config).  M = args.n_matches >= 1; seat (device int32 [N][M]), thrl_crossplay's layout: in
 * match m, seat i is taken by AGENT i OF GAME seat[i][m].  start (device int32 [M]): the tuple index t_0 of match m
 * (the tuple whose price is the state play starts from).
 *
 * Step: t_{k+1} is the index of the tuple (tuple_policy[seat[i][m]][i][t_k])_i.  Entries at or above n_actions_i are
 * clamped to n_actions_i - 1 (the caller's to avoid; nothing is read out of bounds).
 * (mu, lam) are thrl_crossplay's, word for word: mu >= 0, lam >= 1 the smallest values with t_{mu+lam} = t_mu; the
 * cycle is found iff mu + lam <= H (horizon); otherwise lam = 0 and mu = H.  Cycle detection keeps O(1) state per
 * match (Brent) with a step budget that decides "found" exactly by mu + lam <= H.
 * The transition taken at t_k plays the tuple t_{k+1}: its rewards are reward[i][t_{k+1}] and its scaled actions
 * scaled[i][t_{k+1}] (device float64 [N][T] each, the caller's per-config tables).
 *   cycle_reward[i][m] = (sum_{j<lam} reward[i][t_{mu+j+1}], added in that order from 0.0) / lam, cycle_action the
 *   same with scaled; both 0 when lam = 0.  With the tables of tuple_play.tables these are thrl_crossplay's numbers
 *   for the same strategies whenever the two walks visit the same transitions.
 * cycle_start (optional, device int32 [M]): t_mu, or -1 when lam = 0.
 * Rows reward_rows / action_rows [row_count][N][M] (each optional) hold, for tau in [row_begin, row_begin + row_count)
 * inside [0, n_steps), reward[i][t_{tau+1}] and scaled[i][t_{tau+1}]: the layout of the episode rows, so
 * thrl_group_stats reduces them as they are (E = row_count, G = M).
 *
 * A seat outside [0, G) or a start outside [0, T) is device data the host cannot see: that match reads nothing and
 * gets mu = -1, lam = 0, cycle_start = -1 and zeros in cycle_reward, cycle_action and its rows.  No other match is
 * affected.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_matches < 1, n_games < 1, horizon outside [1, THRL_DEV_MAX_HORIZON], n_steps
 * outside [0, THRL_DEV_MAX_STEPS], a row range outside [0, n_steps), reserved != 0, n_tuples < 1 or
 * n_tuples != prod_i n_actions_i; THRL_ERR_UNSUPPORTED for n_tuples > THRL_TP_MAX_TUPLES; THRL_ERR_NULL for a missing
 * cfg, args, seat, start, tuple_policy, reward, scaled, mu, lam, cycle_reward or cycle_action.
 */
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy                    */
    int32_t n_matches;               /* M >= 1                                           */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_steps;                 /* K in [0, THRL_DEV_MAX_STEPS]: length of the path the rows are cut from */
    int32_t horizon;                 /* H >= 1 (th_rl_amd: min(T + 1, 65536))            */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t reserved;                /* 0                                                */
    const int32_t* seat;             /* device [N][M]: game whose agent i sits in match m */
    const int32_t* start;            /* device [M]: start tuple t_0                      */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    int32_t* mu;                     /* device outputs [M]                               */
    int32_t* lam;
    int32_t* cycle_start;            /* device [M] or NULL                               */
    double*  cycle_reward;           /* device [N][M]                                    */
    double*  cycle_action;           /* device [N][M]                                    */
    double*  reward_rows;            /* device [row_count][N][M] or NULL                 */
    double*  action_rows;            /* device [row_count][N][M] or NULL                 */
} thrl_tuple_walk_args;
int thrl_tuple_walk(const thrl_cfg* cfg, const thrl_tuple_walk_args* args, void* stream);

/*
 * Deviation test and equilibrium check in tuple form, for ANY mix of QTable, Reinforce and ActorCritic agents:
 * thrl_deviation and thrl_equilibrium on the arrays thrl_tuple_policy and th_rl_amd.tuple_play.tables produce.  No
 * reference counterpart.  Both calls read tuple_policy (device uint16 [G][N][T], G = args.n_games >= 1), reward (device
 * float64 [N][T]) and start (device int32 [G], the start tuple t_0 of game g, -1 = none); thrl_tuple_deviation also reads
 * scaled (device float64 [N][T]).  Every game is played by its own agents: there is no seat array.  No table, network
 * or price is read and nothing of a batch is written.  Of a valid cfg only n_agents, n_actions and gamma are used.  All
 * arithmetic is float64, every operation rounded once, in the order written here.
 *
 * Tuples are numbered with agent 0 slowest: t = sum_i k_i * prod_{j > i} n_actions_j, T = args.n_tuples =
 * prod_i n_actions_i, 1 <= T <= THRL_TP_MAX_TUPLES.  pi_i(t) = tuple_policy[g][i][t], entries at or above n_actions_i
 * clamped to n_actions_i - 1 (the caller's to avoid; nothing is read out of bounds).  The greedy map is
 * F(t) = the index of the tuple (pi_i(t))_i.
 * THE TRANSITION TAKEN AT t (thrl_tuple_walk's meaning, used by both calls): at t the agents play a tuple u -- F(t) when
 * all are greedy -- and the game moves to u; the reward and scaled action of that transition are reward[i][u] and
 * scaled[i][u].
 *
 * thrl_tuple_deviation: thrl_deviation with "row tuple x" replaced by "tuple index t" and x_0 by start[g].
 * Pre-shock cycle: t_{k+1} = F(t_k); mu >= 0, lam >= 1 the smallest values with t_{mu+lam} = t_mu.  The cycle is found
 * iff mu + lam <= H (horizon); then s* = t_mu.  Otherwise lam = 0, mu = H and s* = t_H (so s* = t_mu in both cases).
 * Cycle detection keeps O(1) state per game (Brent) with a step budget that decides "found" exactly by mu + lam <= H.
 *   cycle_reward[i][g] = (sum_{j<lam} reward_i of the transition taken at F^j(s*), added in that order from 0.0) / lam,
 *   cycle_action the same for the scaled action; both 0 when lam = 0.
 * Deviation path y_0 = s*: for tau < L agent d plays dev_action, or with dev_action = -1 its one-period best response
 * at y_tau: the argmax over k < n_actions_d of reward[d][t'], t' the tuple with k in place d and pi_j(y_tau) in the
 * other places (first maximum under strict >); the others play pi_j(y_tau); y_{tau+1} = the tuple played.  For
 * tau >= L every agent is greedy: y_{tau+1} = F(y_tau).  act_dev[g] = d's action at tau = 0.  Rows reward_rows /
 * action_rows [row_count][N][G] hold, for tau in [row_begin, row_begin + row_count), the rewards and scaled actions of
 * the transition taken at y_tau: the layout of the episode rows, so thrl_group_stats reduces them as they are
 * (E = row_count).  The kernel walks the whole path whatever rows it stores.
 * Baseline path z_0 = s*, every agent greedy.
 * gain[g] = sum_{tau<K} w_tau * (r_d(y_tau) - r_d(z_tau)), r_d(.) agent d's reward of the transition taken there,
 *   w_0 = 1, w_{tau+1} = w_tau * gamma_d, each operation rounded once (subtract, multiply, add);
 *   gamma_d = sweep_gamma[d][g] when given, else cfg.gamma[d].
 * Return: (mu_post, lam_post) = the cycle of F from y_L under the same horizon rule; ret_step[g] = L + mu_post if that
 *   cycle is found and s* lies on it, else -1 (always -1 when lam = 0).
 * A game with start[g] < 0 or start[g] >= T is refused: mu = -1, lam = 0, mu_post = lam_post = 0, ret_step = -1,
 * act_dev = -1, zeros in cycle_reward, cycle_action, gain and its rows.  No other game is affected.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, a deviator outside [0, N), dev_len < 1, n_steps < dev_len or
 * > THRL_DEV_MAX_STEPS, horizon outside [1, THRL_DEV_MAX_HORIZON], dev_action outside {-1} + [0, n_actions[d]), a row
 * range outside [0, n_steps), reserved != 0, n_tuples < 1 or n_tuples != prod_i n_actions_i; THRL_ERR_UNSUPPORTED for
 * n_tuples > THRL_TP_MAX_TUPLES; THRL_ERR_NULL for a missing cfg, args, start, tuple_policy, reward, scaled or per-game
 * output.
 */
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy                    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t deviator;                /* d in [0, N)                                      */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K >= L                                           */
    int32_t horizon;                 /* H >= 1 (th_rl_amd: min(T + 1, 65536))            */
    int32_t dev_action;              /* fixed action index of d, or -1 = best response   */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t reserved;                /* 0                                                */
    const int32_t* start;            /* device [G]: start tuple t_0, outside [0, T) = refused */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    int32_t* mu;                     /* device outputs [G]                               */
    int32_t* lam;
    int32_t* mu_post;
    int32_t* lam_post;
    int32_t* ret_step;
    int32_t* act_dev;
    double*  cycle_reward;           /* device [N][G]                                    */
    double*  cycle_action;           /* device [N][G]                                    */
    double*  gain;                   /* device [G]                                       */
    double*  reward_rows;            /* device [row_count][N][G] or NULL                 */
    double*  action_rows;            /* device [row_count][N][G] or NULL                 */
} thrl_tuple_deviation_args;
int thrl_tuple_deviation(const thrl_cfg* cfg, const thrl_tuple_deviation_args* args, void* stream);

/*
 * thrl_tuple_equilibrium: thrl_equilibrium with the state set replaced by the T tuples, so S = T and state(t) = t.
 * Agent i's problem in game g.  pi_j(s) as above.  t(s, a) = the tuple with a in place i and pi_j(s) elsewhere,
 * R(s, a) = reward[i][t(s, a)] (the reward of the transition taken at s), nxt(s, a) = t(s, a).
 * gamma = sweep_gamma[i][g] when given, else cfg.gamma[i].  Without sweep_gamma, cfg.gamma[i] outside [0, 1) for a
 * selected agent is THRL_ERR_BAD_CONFIG; a game whose sweep gamma is not in [0, 1) is not solved and gets iters = -1,
 * n_diff_all = n_diff_on = 0 and NaN in every float64 output of that agent (br_policy, v_opt, v_pi are not written).
 *
 * Evaluation of a strategy sigma by doubling: V = R(., sigma), n = nxt(., sigma), w = gamma; D times, for all states
 * at once from the old V and n:  V = V + w * V[n];  n = n[n];  w = w * w.   D = the number of squarings w = w * w
 * (from w = gamma) until w < 2^-64, stopping at 64.
 * Policy iteration from the agent's own strategy: sigma_0 = pi_i.  Round k = 0, 1, ..: V_k = evaluation of sigma_k;
 * if k == THRL_EQ_MAX_ITERS stop with iters = -1; Q(s, a) = R(s, a) + gamma * V_k[nxt(s, a)];
 * sigma_{k+1}(s) = sigma_k(s) unless max_a Q(s, a) > Q(s, sigma_k(s)), then the first maximum (strict >, a ascending);
 * if no state changed stop with iters = k.  V_pi = V_0, V* = the last V_k, sigma* = the last strategy.  The incumbent
 * is kept on ties, so a strategy that is a best response gives iters = 0 and V* == V_pi bit for bit.
 *   loss(s) = 0.0 where V*(s) == V_pi(s) or V*(s) == 0, else (V*(s) - V_pi(s)) / V*(s).
 *
 * Path.  t_0 = start[g], t_{k+1} = F(t_k); mu >= 0, lam >= 1 the smallest values with t_{mu+lam} = t_mu:
 * thrl_tuple_walk's mu and lam for a horizon of at least T + 1.  "On path" = the lam tuples t_mu .. t_{mu+lam-1}, in
 * that ("cycle") order.
 *
 * Outputs, per selected agent i (bit i of agents) and game; entries of agents not selected are not written:
 *   iters, n_diff_all, n_diff_on   states / cycle states with sigma*(s) != pi_i(s)
 *   loss_all, loss_on              the largest loss(s) over all states / cycle states
 *   loss_all_mean, loss_on_mean    (sum of loss(s) from 0.0 in state order / cycle order) / T, / lam
 *   v_on                           (sum of V_pi(s) from 0.0 in cycle order) / lam
 *   br_policy, v_opt, v_pi         optional [N][G][T]: sigma*, V*, V_pi per state
 * A game with start[g] < 0 or start[g] >= T has no path: mu = -1, lam = 0, n_diff_on = 0 and NaN in loss_on,
 * loss_on_mean and v_on; its all-states outputs are computed as for any game.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, agents == 0 or with a bit >= N, gamma as above, reserved != 0,
 * n_tuples < 1 or n_tuples != prod_i n_actions_i; THRL_ERR_UNSUPPORTED for n_tuples > THRL_TP_MAX_TUPLES;
 * THRL_ERR_NULL for a missing cfg, args, start, tuple_policy, reward or required output.
 */
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy                    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t agents;                  /* bit i set: solve agent i                         */
    int32_t reserved;                /* 0                                                */
    const int32_t* start;            /* device [G]: start tuple t_0, outside [0, T) = no path */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const double* reward;            /* device [N][T]                                    */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    int32_t* mu;                     /* device [G]                                       */
    int32_t* lam;                    /* device [G]                                       */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* n_diff_all;             /* device [N][G]                                    */
    int32_t* n_diff_on;              /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_on;                /* device [N][G]                                    */
    double*  loss_all_mean;          /* device [N][G]                                    */
    double*  loss_on_mean;           /* device [N][G]                                    */
    double*  v_on;                   /* device [N][G]                                    */
    uint16_t* br_policy;             /* device [N][G][T] or NULL                         */
    double*  v_opt;                  /* device [N][G][T] or NULL                         */
    double*  v_pi;                   /* device [N][G][T] or NULL                         */
} thrl_tuple_equilibrium_args;
int thrl_tuple_equilibrium(const thrl_cfg* cfg, const thrl_tuple_equilibrium_args* args, void* stream);

/*
 * thrl_tuple_attractors: thrl_attractors with the state set replaced by the T tuples, so S = T and state(t) = t: ALL
 * limit cycles of a game's greedy map F on tuple indices and their basins, for ANY mix of QTable, Reinforce and
 * ActorCritic agents.  No reference counterpart.  It follows thrl_tuple_deviation / thrl_tuple_equilibrium: of a valid
 * cfg only n_agents and n_actions are used, there is no seat array, nothing of a batch is read or written, pi_i(t) =
 * tuple_policy[g][i][t] with entries at or above n_actions_i clamped to n_actions_i - 1, F(t) = the index of the tuple
 * (pi_i(t))_i, and the transition taken at t earns reward[i][F(t)] and scaled[i][F(t)] (device float64 [N][T] each).
 * G = args.n_games >= 1, T = args.n_tuples = prod_i n_actions_i, 1 <= T <= THRL_TP_MAX_TUPLES.  All arithmetic is
 * float64, every operation rounded once, in the order written here.
 *
 * For every tuple t: mu(t) = the smallest k >= 0 for which F^k(t) lies on a cycle of F, rep(t) = the smallest tuple
 * index on that cycle, lam = its length.
 *
 * Attractors of a game = the distinct values of rep, n_attr of them.  basin(r) = the number of tuples t with
 * rep(t) = r, the cycle's own tuples included.  Order: basin descending, ties by rep ascending.  The first
 * THRL_ATTR_KEEP are reported, slot k of game g at [k][G] / [k][N][G]:
 *   rep, lam, basin
 *   cycle_reward[k][i][g] = (sum_{j<lam} reward[i][F^{j+1}(rep)], added in that order from 0.0) / lam
 *   cycle_action[k][i][g] = the same with scaled
 * -- the numbers thrl_tuple_walk reports for a walk started at rep.  Slots k >= n_attr get rep = -1, lam = 0,
 * basin = 0 and zeros.  Per game: n_attr, mu_max = max_t mu(t), n_cycle_states = the sum of lam over all attractors,
 * kept or not.
 *
 * Training tuple.  start (device int32 [G]): rep_x0 = rep(start[g]), mu_x0 = mu(start[g]) -- thrl_tuple_walk's mu for
 * a horizon of at least T + 1, and lam of rep_x0's attractor is its lam -- and slot_x0 = that attractor's slot, or -1
 * if it is not among the kept.  A game with start[g] < 0 or start[g] >= T has no training tuple: all three are -1; its
 * other outputs are computed as for any game.
 *
 * Start weights (optional: start_w = NULL skips them, their outputs may then be NULL).  start_w (device float64 [T])
 * holds a weight w_t of every tuple as a starting point; it takes the place of thrl_attractors' reset distribution,
 * which a network would have to be evaluated on a continuum of prices for.  Tuple t reaches the attractor A(t) = the
 * one with rep(t).
 *   start_mass[k][g]    = sum of w_t over the t with A(t) in slot k, start_mass_other[g] over the t whose attractor
 *                         is not kept; both added in ascending t from 0.0
 *   start_reward[i][g]  = sum_t w_t * cycle_reward_i(A(t)) over ALL t, kept or not, in ascending t from 0.0, each
 *                         multiply and each add rounded once
 *
 * tuple_rep, tuple_mu (optional, uint16 [G][T]): rep(t) and mu(t) of every tuple.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, reserved != 0, n_tuples < 1 or n_tuples != prod_i n_actions_i;
 * THRL_ERR_UNSUPPORTED for n_tuples > THRL_TP_MAX_TUPLES; THRL_ERR_NULL for a missing cfg, args, tuple_policy, reward,
 * scaled, start or per-game / per-slot output, or with start_w a missing start_mass, start_mass_other or start_reward.
 */
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy                    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t reserved;                /* 0                                                */
    int32_t reserved2;               /* 0                                                */
    const int32_t* start;            /* device [G]: training tuple, outside [0, T) = none */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* start_w;           /* device [T], or NULL: no start weights            */
    int32_t* n_attr;                 /* device [G]                                       */
    int32_t* mu_max;                 /* device [G]                                       */
    int32_t* n_cycle_states;         /* device [G]                                       */
    int32_t* rep;                    /* device [KEEP][G]                                 */
    int32_t* lam;                    /* device [KEEP][G]                                 */
    int32_t* basin;                  /* device [KEEP][G]                                 */
    double*  cycle_reward;           /* device [KEEP][N][G]                              */
    double*  cycle_action;           /* device [KEEP][N][G]                              */
    int32_t* rep_x0;                 /* device [G]                                       */
    int32_t* mu_x0;                  /* device [G]                                       */
    int32_t* slot_x0;                /* device [G]                                       */
    double*  start_mass;             /* device [KEEP][G], or NULL without start_w        */
    double*  start_mass_other;       /* device [G], or NULL without start_w              */
    double*  start_reward;           /* device [N][G], or NULL without start_w           */
    uint16_t* tuple_rep;             /* device [G][T] or NULL                            */
    uint16_t* tuple_mu;              /* device [G][T] or NULL                            */
} thrl_tuple_attractors_args;
int thrl_tuple_attractors(const thrl_cfg* cfg, const thrl_tuple_attractors_args* args, void* stream);

/*
 * thrl_price_policy: thrl_tuple_policy's contract with a free list of prices in place of the T tuple prices.  No
 * reference counterpart.  price_policy (device uint16 [G][N][J], G = args.n_games in [1, cfg.n_games], J =
 * args.n_prices in [1, THRL_STAT_MAX_CELLS]): entry [g][i][k] is what get_action of agent i of game g returns at the
 * state x[k]:
 *   kind[i] = 0, QTable: the first maximum (strict >) of row encode64_i(x[k]) of agent i's table in q[g];
 *   kind[i] = 1 / 2, Reinforce / ActorCritic: bit for bit the action thrl_nn_act / thrl_ac_act return with u = NULL at
 *     the price (float)x[k] (the evaluation thrl_tuple_policy runs: a game's network stays in a wave's registers while
 *     the wave goes through the game's prices).
 * price (device float64): [J], the same prices for every game, or with THRL_PP_PER_GAME [G][J], x[k] of game g =
 * price[g][k] (J = 1 at a batch's state: the action every agent takes where training stopped).  kind, nn_params and q
 * as in thrl_tuple_policy; everything but price_policy is read only.  Called with the T tuple prices the call writes
 * exactly what thrl_tuple_policy writes.
 *
 * Returns THRL_ERR_UNSUPPORTED for a CAC agent (kind 3) or n_prices > THRL_STAT_MAX_CELLS; THRL_ERR_BAD_CONFIG for
 * n_games outside [1, cfg.n_games], an unknown flag, reserved != 0, a kind outside [0, 3], a neural agent with actions
 * outside [2, 32] or n_prices < 1; THRL_ERR_NULL for a missing cfg, args, price, price_policy, nn_params[i] of a neural
 * agent, or q with a QTable agent in the game.
 */
#define THRL_PP_PER_GAME 1
typedef struct {
    int32_t n_games;                     /* G in [1, cfg.n_games]                            */
    int32_t n_prices;                    /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t flags;                       /* THRL_PP_PER_GAME                                 */
    int32_t reserved;                    /* 0                                                */
    int32_t kind[THRL_MAXA];             /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    const float* nn_params[THRL_MAXA];   /* device [G][P] for the neural agents              */
    const double* price;                 /* device [J], with THRL_PP_PER_GAME [G][J]         */
    uint16_t* price_policy;              /* device [G][N][J], out                            */
} thrl_price_policy_args;
int thrl_price_policy(const thrl_cfg* cfg, const void* q, const thrl_price_policy_args* args, void* stream);

/*
 * thrl_tuple_stationary: greedy play under demand noise (thrl_stationary) for ANY mix of QTable, Reinforce and
 * ActorCritic agents.  No reference counterpart.  Under noise the next price is no tuple's price, but its distribution
 * depends only on the tuple just played: with probability 1 - p it is the tuple's noise-free price, with probability p
 * it is uniform on [0.7 a - u(t), a - u(t)] clipped at 0.  So the distribution over the tuple played at a step is a
 * Markov chain on the game's T action tuples, and this call iterates it.  What it needs beyond tuple_policy is every
 * agent's greedy action as a function of the price on [0, a): a QTable's is piecewise constant with known cuts, a
 * network's is piecewise constant with unknown cuts and is SAMPLED on a per-config grid of cells (thrl_price_policy at
 * the cell midpoints); the share of the axis on which the sampling may be wrong is reported per game (unresolved).
 * Of a valid cfg only n_agents and n_actions are used; nothing of a batch is read or written, every input is read
 * only.  G = args.n_games >= 1, T = args.n_tuples = prod_i n_actions_i <= THRL_TP_MAX_TUPLES, J = args.n_cells in
 * [1, THRL_STAT_MAX_CELLS].  All arithmetic is float64, every operation rounded once, in the order written here.
 *
 * Strategies.  tuple_policy (device uint16 [G][N][T], thrl_tuple_policy) and cell_policy (device uint16 [G][N][J],
 * thrl_price_policy at the cell midpoints); entries at or above n_actions_i are clamped to n_actions_i - 1.  With
 * tstride_i = prod_{j > i} n_actions_j:
 *   F_g(t)   = sum_i min(tuple_policy[g][i][t], A_i - 1) * tstride_i     the tuple played after tuple t without a shock
 *   tau_g(k) = sum_i min(cell_policy[g][i][k], A_i - 1) * tstride_i      the tuple played at a price in cell k
 *
 * Per-config tables, computed by the caller (th_rl_amd.tuple_stationary.tables) and only read here.  Cells: [0, a) cut
 * at {0, a}, at the encode breakpoints of the QTable agents and at a * m / R, m = 1..R-1 (R = the caller's
 * resolution); there are no point cells.  cell_w (device double [J]) = the cell's length / a; the strategies are
 * sampled at the midpoints, which lie strictly inside their cells, so a QTable's entry is exact for its whole cell.
 * reward, scaled (device double [N][T]) and the noise-free price (device double [T]) are th_rl_amd.tuple_play.tables'
 * arrays; band_lo (device int32 [T]), band (device double [T][W], W = band_w), noise_price (device double [T]) and
 * noise_reward (device double [N][T]) are thrl_stationary's "Per-config tables" computed over these cells, with u(t)
 * from tuple_play's quantities: n(t, k) = band[t][k - band_lo[t]] where 0 <= k - band_lo[t] < W, else 0.
 *
 * Noise probability: p_g, q_g = 1 - p_g, the host-visible and the per-game rules of thrl_stationary (an entry of
 * noise_prob_g outside (0, 1], NaN included: that game gets iters = -1 and zeros, no other game is affected).
 *
 * Start distribution over the tuple played first:
 *   m_0(t') = sum over the cells k with tau_g(k) = t' of cell_w(k), in ascending k from 0.0 (the environment's reset,
 *             a uniform price on [0, a)), or
 *   with THRL_TS_START_TUPLE the unit mass on start[g] (device int32 [G]); a value outside [0, T) refuses that game:
 *             iters = -1 and zeros.
 *
 * One step from m, in the lazy form of thrl_stationary:
 *   nu(k)  = sum_t m(t) * n(t, k)                      ascending t from 0.0; terms that are zero may be skipped
 *   D(t')  = sum over the t with F_g(t) = t' of m(t)   ascending t from 0.0
 *   Nn(t') = sum over the k with tau_g(k) = t' of nu(k)   ascending k from 0.0
 *   s(t')  = q_g * D(t') + p_g * Nn(t')
 *   m'(t') = 0.5 * m(t') + 0.5 * s(t')
 *   chg    = max_t |m'(t) - m(t)|
 * Stop after the first step with chg <= args.tol, or after args.max_iters steps.
 *
 * Outputs, per game, from the last iterate m; every sum over ascending t from 0.0:
 *   iters, change        the steps taken and the last chg
 *   mass                 sum_t m(t)
 *   stat_reward[i][g]    sum_t m(t) * (q_g * reward_i(t) + p_g * noise_reward_i(t))
 *   stat_action[i][g]    sum_t m(t) * scaled_i(t)
 *   stat_price[g]        sum_t m(t) * (q_g * price(t) + p_g * noise_price(t))
 *   pi (optional, double [G][T])   m itself
 *
 * Diagnostics of the sampling (optional, each may be NULL), from cell_policy alone and for every game, refused or not.
 * kind[i] (thrl_tuple_policy's codes) says which agents are networks:
 *   n_switch[g]    the number of pairs of adjacent cells (k, k + 1) on which the clamped entry of some neural agent
 *                  differs
 *   unresolved[g]  sum over those pairs of 0.5 * (cell_w(k) + cell_w(k + 1)), in ascending k from 0.0: the share of the
 *                  price axis on which a sampled network strategy may differ from the true one
 * A strategy that switches twice between two adjacent midpoints is not seen by either; a finer grid is the remedy.
 *
 * Working set.  A game is solved by one block in LDS: the two iterates and nu (16 T + 8 J bytes), the stable groupings
 * of the cells by tau_g and of the tuples by F_g (2 J + 6 T + 4 bytes) and 512 (2 N + 2) bytes of staging, the sum
 * rounded up to 16 bytes: 22 T + 10 J + 512 (2 N + 2) + 4.  The call returns THRL_ERR_UNSUPPORTED when that exceeds a
 * CU's LDS; on a 160 KB CU it does not within the limits on T and J (131.0 KB at T = J = 4096 with two agents,
 * 137.0 KB with eight), so every game within them is solved.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, an unknown flag, n_tuples < 1 or n_tuples != prod_i n_actions_i,
 * n_cells < 1, band_w < 1, max_iters outside [1, THRL_STAT_MAX_ITERS], tol < 0 or NaN, noise_prob as above, or a kind
 * outside [0, 3]; THRL_ERR_UNSUPPORTED for a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES, n_cells >
 * THRL_STAT_MAX_CELLS or the working set; THRL_ERR_NULL for a missing cfg, args, tuple_policy, cell_policy, table
 * (cell_w, reward, scaled, price, band_lo, band, noise_reward, noise_price), per-game output other than pi, n_switch and
 * unresolved, or start with THRL_TS_START_TUPLE.
 */
#define THRL_TS_START_TUPLE 1
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy and cell_policy    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t max_iters;               /* in [1, THRL_STAT_MAX_ITERS]                      */
    int32_t flags;                   /* THRL_TS_START_TUPLE                              */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic: read for n_switch / unresolved */
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  tol;                     /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const int32_t* start;            /* device [G], with THRL_TS_START_TUPLE             */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const uint16_t* cell_policy;     /* device [G][N][J]                                 */
    const double* cell_w;            /* device [J]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* price;             /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* noise_price;       /* device [T]                                       */
    int32_t* iters;                  /* device [G]                                       */
    double*  change;                 /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  stat_reward;            /* device [N][G]                                    */
    double*  stat_action;            /* device [N][G]                                    */
    double*  stat_price;             /* device [G]                                       */
    double*  pi;                     /* device [G][T] or NULL                            */
    int32_t* n_switch;               /* device [G] or NULL                               */
    double*  unresolved;             /* device [G] or NULL                               */
} thrl_tuple_stationary_args;
int thrl_tuple_stationary(const thrl_cfg* cfg, const thrl_tuple_stationary_args* args, void* stream);

/*
 * thrl_tuple_equilibrium_noise: the equilibrium check under demand noise (thrl_equilibrium_noise) for ANY mix of
 * QTable, Reinforce and ActorCritic agents: is agent i's strategy a best response to the rivals' strategies in the
 * environment of thrl_tuple_stationary, and which share of the attainable value does it give up if not.  No reference
 * counterpart.  The world is thrl_tuple_stationary's, unchanged: the action tuples t < T = args.n_tuples, tuple_policy
 * [G][N][T] (the strategies evaluated exactly at each tuple's noise-free price), cell_policy [G][N][J] (the strategies
 * sampled at the midpoints of the J = args.n_cells cells), the per-config tables reward, band_lo, band (W = band_w) and
 * noise_reward, n(t, k), p_g and q_g = 1 - p_g with thrl_stationary's host-visible and per-game rules; entries of the
 * strategies at or above n_actions_i are clamped to n_actions_i - 1.  Of a valid cfg only n_agents and n_actions are
 * used; nothing of a batch is read or written, every input is read only.  All arithmetic is float64, every operation
 * rounded once, in the order written here.
 *
 * States.  An agent sees the price.  The prices that occur are the T noise-free tuple prices, each reached with
 * probability q after its tuple, and the continuum reached after a shock, lumped into the J cells.  The state set is
 * S = T + J, the tuple-states first: state s < T is tuple-state t = s, state s >= T is cell-state k = s - T.
 *   tuple-state t: the price is exactly tuple t's; the tuple played there is F_g(t) (thrl_tuple_stationary)
 *   cell-state k:  the price lies in cell k; the tuple played there is tau_g(k)
 * A value function V has the parts V_T [T] and V_J [J].  pi_i(s) = agent i's action in the tuple played at s;
 * t(s, a) = that tuple with a in place i.  Agent i's problem in game g, with p = p_g, q = q_g, gamma =
 * sweep_gamma[i][g] when given, else args.gamma[i] (without sweep_gamma an args.gamma[i] outside [0, 1) of a selected
 * agent is THRL_ERR_BAD_CONFIG; cfg.gamma is not read: a network's gamma is not the placeholder table slot's):
 *   R(s, a) = q * reward_i(t) + p * noise_reward_i(t)  with t = t(s, a)
 *   z_V(t)  = q * V_T[t] + p * b,  b = the sum over w = 0 .. W-1, ascending, from 0.0, of
 *             band[t][w] * V_J[band_lo[t] + w]; terms whose cell band_lo[t] + w lies outside [0, J) are skipped.
 * Both depend on the tuple alone.
 *
 * Solver: thrl_equilibrium_noise's, word for word, with s over the S states in place of its cells k: the evaluation of
 * a strategy by Jacobi sweeps, V^{m+1}(s) = R(s, sigma(s)) + gamma * z_{V^m}(t(s, sigma(s))), chg_m = max_s |V^{m+1}(s)
 * - V^m(s)|, stopped after the first sweep with chg <= eval_tol and CAPPED after max_sweeps sweeps without that; policy
 * iteration from sigma_0 = pi_i and V^0 = 0 (the previous round's V after round 0) with Q(s, a) = R(s, a) + gamma *
 * z_{V_n}(t(s, a)), margin = ((2 * gamma) * gamma) * eval_tol / (1 - gamma), the keep-the-incumbent / first-maximum
 * rule, the cap THRL_EQ_MAX_ITERS on the rounds, V_pi = V_0, V* = the last V_n, sigma* = the last strategy and
 *   loss(s) = 0.0 where V*(s) == V_pi(s) or V*(s) == 0, else (V*(s) - V_pi(s)) / V*(s).
 * A best response may act differently at a tuple's exact price than in the cell around it: the two are different
 * states, in which the rivals (whose strategies are sampled at the cell's midpoint) may act differently too.
 *
 * Outputs, per selected agent i (bit i of agents) and game; entries of agents not selected are not written:
 *   iters, sweeps      the rounds n (-1 when not solved) and all evaluation sweeps of the (agent, game)
 *   n_diff_tuples      tuple-states with sigma*(s) != pi_i(s);  n_diff_cells the same over the cell-states
 *   loss_all           the largest loss(s) over all S states
 *   loss_tuples_mean   (sum of loss(s) over the tuple-states, ascending from 0.0) / T
 *   loss_cells_mean    (sum of loss(s) over the cell-states, ascending from 0.0) / J
 *   with pi (device double [G][T], thrl_tuple_stationary's long-run distribution over the tuple played, finite; NULL:
 *   the three outputs are not written) the weights say where decisions are made in the long run:
 *     w(t) = q_g * pi(t) at tuple-state t;  w(k) = p_g * nu(k) at cell-state k, nu(k) = the sum over ascending t from 0.0
 *     of pi(t) * n(t, k) over the t with 0 <= k - band_lo[t] < W (elsewhere n(t, k) = 0: the term is skipped)
 *     loss_w = sum w(s) * loss(s),  diff_w = sum of w(s) over the states with sigma*(s) != pi_i(s) (+0.0 elsewhere),
 *     v_w = sum w(s) * V_pi(s); each one sum from 0.0 over the tuple-states first, then the cells, ascending
 *   br_policy (uint16), v_opt, v_pi   optional [N][G][S]: sigma*, V*, V_pi per state, tuple-states first
 *
 * Games that are not solved, as in thrl_equilibrium_noise; no other game is affected.  An entry of noise_prob_g outside
 * (0, 1] (NaN included): iters = -1 and zeros in every output of every selected agent, the optional ones included.
 * Otherwise a gamma outside [0, 1) (NaN included), or a capped (agent, game): iters = -1, n_diff_tuples = n_diff_cells
 * = 0, sweeps = the sweeps made, NaN in every float64 output of that agent, and br_policy = pi_i.
 *
 * Working set.  A game is solved by one wavefront in LDS: three value arrays over the states (24 S bytes), the tuple
 * played at a state by the incumbent and by the current strategy (4 S), R and R + gamma * z per tuple (16 T) and 2,048
 * bytes of staging, the sum rounded up to 16 bytes: 44 T + 28 J + 2048.  A sweep computes z once per tuple (T (W + 1)
 * multiply-adds) and reads it back per state.  Above THRL_TEN_MAX_LDS = 160 KB (a CU's LDS on CDNA4), or the device's
 * own limit, the call returns THRL_ERR_UNSUPPORTED without launching: T = 441 with J = 4096 fits (136,144 bytes), T = J
 * = 2,247 fits, T = J = 4096 (296,960 bytes) does not.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, flags or reserved != 0, agents == 0 or with a bit >= N, a kind outside
 * [0, 3], n_tuples < 1 or n_tuples != prod_i n_actions_i, gamma as above, n_cells < 1, band_w < 1, max_sweeps outside
 * [1, THRL_STAT_MAX_ITERS], eval_tol < 0 or NaN, or a host-visible noise_prob outside (0, 1]; THRL_ERR_UNSUPPORTED for
 * a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES, n_cells > THRL_STAT_MAX_CELLS or the working set; THRL_ERR_NULL
 * for a missing cfg, args, tuple_policy, cell_policy, table (reward, band_lo, band, noise_reward), iters, sweeps,
 * n_diff_tuples, n_diff_cells, loss_all, loss_tuples_mean or loss_cells_mean, or with pi a missing loss_w, diff_w or v_w.
 */
#define THRL_TEN_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy and cell_policy    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t max_sweeps;              /* in [1, THRL_STAT_MAX_ITERS], per evaluation      */
    int32_t agents;                  /* bit i set: solve agent i                         */
    int32_t flags;                   /* 0                                                */
    int32_t reserved;                /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic       */
    double  gamma[THRL_MAXA];        /* in [0, 1), read when sweep_gamma is NULL         */
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  eval_tol;                /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const uint16_t* cell_policy;     /* device [G][N][J]                                 */
    const double* reward;            /* device [N][T]                                    */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* pi;                /* device [G][T] or NULL                            */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* sweeps;                 /* device [N][G]                                    */
    int32_t* n_diff_tuples;          /* device [N][G]                                    */
    int32_t* n_diff_cells;           /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_tuples_mean;       /* device [N][G]                                    */
    double*  loss_cells_mean;        /* device [N][G]                                    */
    double*  loss_w;                 /* device [N][G], with pi                           */
    double*  diff_w;                 /* device [N][G], with pi                           */
    double*  v_w;                    /* device [N][G], with pi                           */
    uint16_t* br_policy;             /* device [N][G][T + J] or NULL                     */
    double*  v_opt;                  /* device [N][G][T + J] or NULL                     */
    double*  v_pi;                   /* device [N][G][T + J] or NULL                     */
} thrl_tuple_equilibrium_noise_args;
int thrl_tuple_equilibrium_noise(const thrl_cfg* cfg, const thrl_tuple_equilibrium_noise_args* args, void* stream);

/*
 * thrl_tuple_deviation_noise: the deviation test under demand noise (thrl_deviation_noise) for ANY mix of QTable,
 * Reinforce and ActorCritic agents: does a deviation pay, do the others punish, does play return, in expectation, in
 * the environment of thrl_tuple_stationary.  No reference counterpart.  Under noise greedy play follows no single path
 * of tuples, so the answer is the propagation of a distribution: the tuple greedy play intends at a period is a Markov
 * chain on the T action tuples, a forced deviation replaces the deviator's action in the tuple actually played for L
 * periods, and the response is the sequence of distributions that follow from the one the shock hits.  No sampling.
 * The world is thrl_tuple_stationary's, unchanged: the action tuples t < T = args.n_tuples, the J = args.n_cells cells,
 * tuple_policy [G][N][T] and cell_policy [G][N][J] with F_g, tau_g, the clamping rule and tstride, the per-config tables
 * reward, scaled, band_lo, band (W = band_w) and noise_reward, n(t, k), p_g and q_g = 1 - p_g with the host-visible and
 * the per-game rules.  cell_w, price and noise_price are not read.  Of a valid cfg only n_agents, n_actions and gamma
 * are used; nothing of a batch is read or written, every input is read only.  All arithmetic is float64, every
 * operation rounded once, in the order written here; every sum runs over ascending index from 0.0.
 *
 *   R_i(u)    = q_g * reward_i(u) + p_g * noise_reward_i(u)   (thrl_tuple_stationary's expected reward)
 *   Dv_g(t)   = t with the deviator d's action replaced, a map on tuples: by dev_action, or with dev_action = -1 by
 *               d's one-period best response to the rivals' actions in t, the argmax over a < A_d of R_d(t with a in
 *               place d), the first maximum under strict >.  With per-game noise Dv is per game
 *   e_tau(t)  = Dv_g(t) for tau < L, t afterwards: the tuple actually played when greedy play intends t
 *   m_tau(t)  = the probability that the tuple greedy play intends at period tau is t
 *   m_0       = weights[g] (device double [G][T], required): the distribution the shock hits, e.g.
 *               thrl_tuple_stationary's pi
 *   the plain step, not the lazy one, so the iterate after tau steps is the distribution at period tau:
 *     nu(k)   = sum_t m_tau(t) * n(e_tau(t), k)                       terms that are zero may be skipped
 *     D(t')   = sum over the t with F_g(e_tau(t)) = t' of m_tau(t)
 *     Nn(t')  = sum over the k with tau_g(k) = t' of nu(k)
 *     m_{tau+1}(t') = q_g * D(t') + p_g * Nn(t')                      two products, one add
 *   E_i(tau)  = sum_t m_tau(t) * R_i(e_tau(t)),  A_i(tau) = sum_t m_tau(t) * scaled_i(e_tau(t))
 *   Dist(tau) = 0.5 * sum_t |m_tau(t) - m_0(t)|: the total-variation distance from the start (Dist(0) = 0)
 *
 * Rows reward_rows / action_rows [row_count][N][G] (optional) hold E_i(tau) / A_i(tau) for tau in [row_begin, row_begin +
 * row_count): the layout of the episode rows, so thrl_group_stats reduces them as they are (E = row_count); dist_rows
 * [row_count][G] (optional) holds Dist(tau).  The kernel walks all K periods whatever rows it stores.
 *
 * Outputs, per game:
 *   base_reward[i][g] = sum_t m_0(t) * R_i(t): the expression of thrl_tuple_stationary's stat_reward, bit-equal to it
 *                       with its pi as weights;  base_action[i][g] = sum_t m_0(t) * scaled_i(t)
 *   dev_share[g]      = the sum of m_0(t) over the tuples with Dv_g(t) != t (+0.0 elsewhere): the long-run share of
 *                       periods in which the deviation changes anything
 *   gain[g]           = sum_{tau<K} w_tau * (E_d(tau) - base_reward_d), w_0 = 1, w_{tau+1} = w_tau * gamma_d (subtract,
 *                       multiply, add); gamma_d = sweep_gamma[d][g] when given, else cfg.gamma[d]
 *   gain_dev[g]       = the same sum over tau < L: what the deviation itself earns; gain - gain_dev is the aftermath
 *   low[g]            = min_{L <= tau < K} (E_d(tau) - base_reward_d), low_step[g] its first tau; K == L: 0.0 and -1
 *   ret_step[g]       = the first tau in [L, K] with Dist(tau) <= ret_tol, else -1
 *   dist[g] = Dist(K),  mass[g] = sum_t m_K(t)
 * A game whose noise_prob_g entry lies outside (0, 1] (NaN included) gets zeros in every float64 output, its rows
 * included, and -1 in low_step and ret_step; no other game is affected.
 *
 * Working set.  A game is solved by one block in LDS: the two iterates and nu (16 T + 8 J bytes), the stable groupings
 * of the cells by tau_g, of the tuples by F_g o Dv_g and of the tuples by F_g (2 J + 10 T + 6 bytes), Dv_g (2 T) and
 * 512 (2 N + 2) bytes of staging, the sum rounded up to 16 bytes: 28 T + 10 J + 512 (2 N + 2) + 6.  Above
 * THRL_TDN_MAX_LDS = 160 KB (a CU's LDS on CDNA4), or the device's own limit, the call returns THRL_ERR_UNSUPPORTED
 * without launching; with two agents it does not within the limits on T and J (158,736 bytes at T = J = 4096), so every
 * two-agent game thrl_tuple_stationary solves is solved here.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, flags or reserved != 0, a kind outside [0, 3], n_tuples < 1 or n_tuples
 * != prod_i n_actions_i, a deviator outside [0, N), dev_len < 1, n_steps < dev_len or > THRL_DEV_MAX_STEPS, dev_action
 * outside {-1} + [0, n_actions[d]), a row range outside [0, n_steps), n_cells < 1, band_w < 1, ret_tol < 0 or NaN, or a
 * host-visible noise_prob outside (0, 1]; THRL_ERR_UNSUPPORTED for a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES,
 * n_cells > THRL_STAT_MAX_CELLS or the working set; THRL_ERR_NULL for a missing cfg, args, tuple_policy, cell_policy,
 * table (reward, scaled, band_lo, band, noise_reward), weights or per-game output.  All of these are decided before
 * any launch.
 */
#define THRL_TDN_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of tuple_policy and cell_policy    */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_cells;                 /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t deviator;                /* d in [0, N)                                      */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K >= L                                           */
    int32_t dev_action;              /* fixed action index of d, or -1 = best response   */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t flags;                   /* 0                                                */
    int32_t reserved;                /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic       */
    double  noise_prob;              /* p in (0, 1], read when noise_prob_g is NULL      */
    double  ret_tol;                 /* >= 0                                             */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const uint16_t* tuple_policy;    /* device [G][N][T]                                 */
    const uint16_t* cell_policy;     /* device [G][N][J]                                 */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* weights;           /* device [G][T] (required): m_0                    */
    double*  base_reward;            /* device [N][G]                                    */
    double*  base_action;            /* device [N][G]                                    */
    double*  dev_share;              /* device [G]                                       */
    double*  gain;                   /* device [G]                                       */
    double*  gain_dev;               /* device [G]                                       */
    double*  low;                    /* device [G]                                       */
    int32_t* low_step;               /* device [G]                                       */
    int32_t* ret_step;               /* device [G]                                       */
    double*  dist;                   /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  reward_rows;            /* device [row_count][N][G] or NULL                 */
    double*  action_rows;            /* device [row_count][N][G] or NULL                 */
    double*  dist_rows;              /* device [row_count][G] or NULL                    */
} thrl_tuple_deviation_noise_args;
int thrl_tuple_deviation_noise(const thrl_cfg* cfg, const thrl_tuple_deviation_noise_args* args, void* stream);

/*
 * thrl_price_probs: the action PROBABILITIES of the neural agents at a free list of prices, where thrl_price_policy
 * gives their greedy action.  No reference counterpart.  For every agent i with kind[i] = 1 / 2 (Reinforce /
 * ActorCritic) the call writes prob[i] (device float32 [G][J][A_i], G = args.n_games in [1, cfg.n_games], J =
 * args.n_prices in [1, THRL_STAT_MAX_CELLS]): row [g][k] is bit for bit the vector thrl_nn_act / thrl_ac_act return in
 * prob_out for game g at the price (float)x[k] -- the softmax training samples from (agents.py:148-163), evaluated by
 * the same device function with the same padding, a game's network held in a wave's registers while the wave goes
 * through the J prices.  price (device float64 [J]) is shared by the games.  QTable agents (kind 0) are skipped: their
 * prob[i] and nn_params[i] are not read; their greedy entry at the same prices is thrl_price_policy's.  Of a valid cfg
 * only n_games, n_agents and n_actions are used; everything but prob[i] is read only.
 *
 * Returns THRL_ERR_UNSUPPORTED for a CAC agent (kind 3) or n_prices > THRL_STAT_MAX_CELLS; THRL_ERR_BAD_CONFIG for
 * n_games outside [1, cfg.n_games], flags != 0, reserved != 0, a kind outside [0, 3], a neural agent with actions
 * outside [2, 32] or n_prices < 1; THRL_ERR_NULL for a missing cfg, args, price, or nn_params[i] / prob[i] of a neural
 * agent.
 */
typedef struct {
    int32_t n_games;                     /* G in [1, cfg.n_games]                            */
    int32_t n_prices;                    /* J in [1, THRL_STAT_MAX_CELLS]                    */
    int32_t flags;                       /* 0                                                */
    int32_t reserved;                    /* 0                                                */
    int32_t kind[THRL_MAXA];             /* 0 = QTable (skipped), 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    const float* nn_params[THRL_MAXA];   /* device [G][P] for the neural agents              */
    const double* price;                 /* device [J]                                       */
    float* prob[THRL_MAXA];              /* device [G][J][A_i] for the neural agents, out    */
} thrl_price_probs_args;
int thrl_price_probs(const thrl_cfg* cfg, const thrl_price_probs_args* args, void* stream);

/*
 * thrl_sampled_chain: SAMPLED play, the exact long-run profit of the stochastic policies the agents were trained
 * with, where every other analysis call treats an agent as its greedy policy.  No reference counterpart (the closest is
 * play_game with the commented-out sample_action, utils.py:36-39).  Without demand noise the price after a step is a
 * function of the action tuple just played, so under sampling the tuple played at a step is a Markov chain on the
 * game's T tuples with P(t -> t') = prod_i pi_i(a_i(t') | price(t)), and this call iterates it.  The transition row
 * depends on t only through price(t), so everything is indexed by the D <= T DISTINCT prices of the config; the row is
 * a product over agents, so a step costs T D N multiplications and needs D sum_i A_i probabilities, never a T x T
 * matrix.  Of a valid cfg only n_agents and n_actions are used; nothing of a batch is read or written, every input is
 * read only.  G = args.n_games >= 1, T = args.n_tuples = prod_i n_actions_i <= THRL_TP_MAX_TUPLES, D = args.n_prices in
 * [1, T].  a_i(t) = (t / tstride_i) mod A_i with tstride_i = prod_{j > i} n_actions_j (agent 0 slowest).  All
 * arithmetic is float64, every operation is rounded once (no contraction), in the order written here.
 *
 * Per-config tables, computed by the caller (th_rl_amd.sampled_play.tables) and only read here; no device arithmetic
 * produces any of them.  dprice [D]: the distinct values of tuple_play's price [T], ascending (two prices are equal
 * when their float64 bits are equal); it is what the caller hands to thrl_price_probs and thrl_price_policy and is not
 * an argument here.  row(t) = the index of price(t) in dprice, given as its stable grouping: grp_first (device int32
 * [D + 1]) and grp_perm (device int32 [T]): the tuples with row(t) = d are grp_perm[grp_first[d] .. grp_first[d + 1])
 * in ascending t.  The device clamps grp_first to [0, T] and grp_perm to [0, T) when it stages them, so no entry leads
 * out of bounds.  reward, scaled (device double [N][T]) and price (device double [T]) are tuple_play's arrays.
 *
 * Inputs per game.  prob[i] for the neural agents (kind[i] = 1 / 2): device float32 [G][D][A_i], thrl_price_probs at
 * dprice.  dpolicy (device uint16 [G][N][D]), thrl_price_policy at dprice: read for the QTable agents and for `agree`;
 * entries are clamped to A_i - 1: g_i(d) = min(dpolicy[g][i][d], A_i - 1).  eps[i] scalars, or eps_g (device double
 * [N][G]) which then replaces them: the exploration rate of the QTable agents (the entries of neural agents are not
 * read).  A scalar outside [0, 1] (NaN included) for a QTable agent is THRL_ERR_BAD_CONFIG; such an entry of eps_g is
 * device data and refuses that game only: iters = -1 and zeros, no other game is affected.
 *
 * Probabilities.
 *   neural agent:  P_i(k|d) = (double)prob[i][g][d][k];  S_i(d) = sum_k P_i(k|d), ascending k from 0.0
 *   QTable agent (agents.py:80-89, random.choice over ALL actions):  lo = eps / A_i;
 *                  P_i(k|d) = (1 - eps) + lo for k = g_i(d), else lo;  S_i(d) = 1.0 exactly
 *   Z(d) = S_0(d) * S_1(d) * ...   multiplied left to right
 * The float32 softmax rows do not sum to one; the division by Z keeps the chain's mass from drifting over thousands of
 * steps.
 *
 * Start.  m_0 = 1 / T on every tuple, or with THRL_SP_START_TUPLE the unit mass on start[g] (device int32 [G]); a
 * value outside [0, T) refuses that game: iters = -1 and zeros.
 *
 * One step from m, in thrl_stationary's lazy form (with eps = 0 tables the chain is a deterministic map and may be
 * periodic):
 *   M(d)   = sum over the t with row(t) = d of m(t)          ascending t from 0.0
 *   W(d)   = M(d) / Z(d)
 *   s(t')  = sum_d ((W(d) * P_0(a_0(t')|d)) * P_1(a_1(t')|d)) * ...      ascending d from 0.0; a d with W(d) == 0.0 is
 *            skipped (M(d) == 0: its terms are +0.0)
 *   m'(t') = 0.5 * m(t') + 0.5 * s(t')
 *   chg    = max_t |m'(t) - m(t)|
 * Stop after the first step with chg <= args.tol, or after args.max_iters steps.
 *
 * Outputs, per game, from the last iterate m (M and W recomputed from it); every sum in ascending index from 0.0:
 *   iters, change        the steps taken and the last chg
 *   mass                 sum_t m(t)
 *   samp_reward[i][g]    sum_t m(t) * reward_i(t)
 *   samp_action[i][g]    sum_t m(t) * scaled_i(t)
 *   samp_price[g]        sum_t m(t) * price(t)
 *   agree[g]             sum_d ((W(d) * P_0(g_0(d)|d)) * P_1(g_1(d)|d)) * ...   every d, none skipped: the long-run share
 *                        of steps on which every agent plays its greedy action
 *   pi (optional, double [G][T])   m itself
 *
 * Working set.  A game is solved by one 256-thread block in LDS: the two iterates (16 T bytes), W and Z (16 D), the
 * float32 probability rows of the neural agents (4 D A_i each, row-major [d][k], so lanes with consecutive a_{N-1} read
 * consecutive words), 2 bytes per (QTable agent, d), the grouping (2 (D + 1) + 2 T), 512 (2 N + 2) bytes of staging
 * for the ordered output sums and 256 bytes of per-game constants, each array rounded up to 16 bytes:
 *   sum of r16(x) over x in { 8 T, 8 T, 8 D, 8 D, 4 D A_i (neural i), 2 D (QTable i), 2 (D + 1), 2 T, 512 (2 N + 2), 256 }
 * The call returns THRL_ERR_UNSUPPORTED, without launching, when that exceeds THRL_SP_MAX_LDS = 160 KB (a CU's LDS on
 * gfx950) or the device's own limit.  QTable 21 x Reinforce 21 (T = D = 441) takes 57,216 bytes, 2 x Reinforce 21 on
 * one exact grid (T = 441, D = 41) 18,976; against a 32-action network a QTable of 30 actions (T = D = 960, 162,704
 * bytes) fits and one of 32 (T = D = 1024) does not.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, an unknown flag, reserved != 0, n_tuples < 1 or n_tuples != prod_i
 * n_actions_i, n_prices outside [1, n_tuples], max_iters outside [1, THRL_STAT_MAX_ITERS], tol < 0 or NaN, eps as
 * above, or a kind outside [0, 3]; THRL_ERR_UNSUPPORTED for a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES or the
 * working set; THRL_ERR_NULL for a missing cfg, args, prob[i] of a neural agent, dpolicy, table (grp_first, grp_perm,
 * reward, scaled, price), per-game output other than pi, or start with THRL_SP_START_TUPLE.
 */
#define THRL_SP_START_TUPLE 1
#define THRL_SP_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of prob and dpolicy                */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t max_iters;               /* in [1, THRL_STAT_MAX_ITERS]                      */
    int32_t flags;                   /* THRL_SP_START_TUPLE                              */
    int32_t reserved;                /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  tol;                     /* >= 0                                             */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const int32_t* start;            /* device [G], with THRL_SP_START_TUPLE             */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* price;             /* device [T]                                       */
    int32_t* iters;                  /* device [G]                                       */
    double*  change;                 /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  samp_reward;            /* device [N][G]                                    */
    double*  samp_action;            /* device [N][G]                                    */
    double*  samp_price;             /* device [G]                                       */
    double*  agree;                  /* device [G]                                       */
    double*  pi;                     /* device [G][T] or NULL                            */
} thrl_sampled_chain_args;
int thrl_sampled_chain(const thrl_cfg* cfg, const thrl_sampled_chain_args* args, void* stream);

/*
 * thrl_sampled_noise_chain: sampled play UNDER DEMAND NOISE, the environment the reference ships
 * (NoisyPriceState, noise_prob = 0.05): thrl_sampled_chain's chain of stochastic policies combined with
 * thrl_tuple_stationary's model of the redrawn price.  With probability q = 1 - p the price after tuple t is its
 * noise-free price (one of the D distinct prices); with probability p it is uniform on [0.7 a - u(t), a - u(t)) clipped
 * at 0, where a network's probabilities live on a continuum: they are taken at Jn quadrature NODES.  Of a valid cfg
 * only n_agents and n_actions are used; nothing of a batch is read or written, every input is read only.  G, T, D,
 * a_i(t) and the ground rules are thrl_sampled_chain's: all arithmetic float64, every operation rounded once, every sum
 * in the order written here.
 *
 * Nodes, computed by the caller (th_rl_amd.sampled_play.noise_tables) and only read here.  xn[0] = 0.0, the atom of the
 * prices clipped to 0; xn[1 + k] = cell_x[k], the midpoints of thrl_tuple_stationary's J cells: Jn = args.n_nodes =
 * J + 1 in [2, THRL_STAT_MAX_CELLS].  xn is what the caller hands to thrl_price_probs and thrl_price_policy and is not
 * an argument here.  nn(t, 0) = z(t) / width, nn(t, 1 + k) = len_k(t) / width with thrl_tuple_stationary's len_k, z and
 * width (the clipped mass has its own node instead of being lumped into cell 0), given as band_lo (device int32 [T]) and
 * band (device double [T][W], W = args.band_w >= 1): nn(t, j) = band[t][j - band_lo[t]] for band_lo[t] <= j <
 * band_lo[t] + W, else 0; any band_lo is safe.  noise_price (device double [T]) and noise_reward (device double [N][T])
 * are thrl_tuple_stationary's.  node_w (device double [Jn]): 0 for the atom, cell_w for the cells.  grp_first,
 * grp_perm, reward, scaled and price are thrl_sampled_chain's.
 *
 * Inputs per game.  prob[i], dpolicy, eps / eps_g exactly as in thrl_sampled_chain.  nprob[i] for the neural agents:
 * device float32 [G][Jn][A_i], thrl_price_probs at xn (4-byte alignment suffices).  npolicy (device uint16 [G][N][Jn]),
 * thrl_price_policy at xn, gn_i(j) = min(npolicy[g][i][j], A_i - 1): a QTable agent's greedy action is exact on every
 * node (the atom sits in the row of cell 0).  noise_prob, or noise_prob_g (device double [G]) which then replaces it:
 * p in [0, 1], zero allowed.  A scalar outside [0, 1] (NaN included) is THRL_ERR_BAD_CONFIG; such an entry of
 * noise_prob_g or eps_g refuses that game only: iters = -1 and zeros.
 *
 * Probabilities.  P_i(k|d), S_i(d), Z(d) are thrl_sampled_chain's; Pn_i(k|j), Sn_i(j), Zn(j) are the same definitions
 * on the node rows (nprob, gn).
 *
 * Start.  m_0 = 1 / T on every tuple; with THRL_SPN_START_TUPLE the unit mass on start[g] (outside [0, T): refused);
 * with THRL_SPN_START_RESET the tuple played at a uniform price on [0, a):
 *   m_0(t') = sum_j (((node_w(j) / Zn(j)) * Pn_0(a_0(t')|j)) * Pn_1(a_1(t')|j)) * ...   ascending j from 0.0, a j with
 *             node_w(j) == 0 skipped
 *
 * One step from m:
 *   M(d)   = sum over the t with row(t) = d of m(t)         ascending t from 0.0;   W(d) = M(d) / Z(d)
 *   nu(j)  = sum_t m(t) * nn(t, j)                          ascending t from 0.0 (zero terms change nothing);
 *   V(j)   = nu(j) / Zn(j)
 *   Sd(t') = sum_d ((W(d) * P_0(a_0(t')|d)) * P_1(a_1(t')|d)) * ...      ascending d, a d with W(d) == 0.0 skipped
 *   Sn(t') = sum_j ((V(j) * Pn_0(a_0(t')|j)) * Pn_1(a_1(t')|j)) * ...    ascending j, a j with V(j) == 0.0 skipped
 *   s(t')  = q * Sd(t') + p * Sn(t')                        q = 1 - p
 *   m'(t') = 0.5 * m(t') + 0.5 * s(t');   chg = max_t |m'(t) - m(t)|
 * Stop after the first step with chg <= args.tol, or after args.max_iters steps.  With p = 0, s = 1.0 * Sd + 0.0 * Sn =
 * Sd exactly: every output then has the bits of thrl_sampled_chain.
 *
 * Outputs, per game, from the last iterate (M, W, nu, V recomputed from it), every sum in ascending index from 0.0:
 *   iters, change, mass  as in thrl_sampled_chain
 *   samp_reward[i][g]    sum_t m(t) * (q * reward_i(t) + p * noise_reward_i(t))
 *   samp_action[i][g]    sum_t m(t) * scaled_i(t)
 *   samp_price[g]        sum_t m(t) * (q * price(t) + p * noise_price(t))
 *   agree[g]             q * (sum_d ((W(d) * P_0(g_0(d)|d)) * ...)) + p * (sum_j ((V(j) * Pn_0(gn_0(j)|j)) * ...)),
 *                        every index included
 *   pi (optional, double [G][T])   m itself
 *   max_jump (optional, double [G]), for EVERY game, refused or not: the maximum over the neural agents i, the adjacent
 *                        nodes 1 <= j < Jn - 1 and the actions k of |Pn_i(k|j + 1) - Pn_i(k|j)| (the difference of the
 *                        two float32 values in float64); 0 without a neural agent.  It is the midpoint rule's honesty
 *                        figure: the quadrature takes a network's row as constant across a cell.
 *
 * Working set.  One 256-thread block per game in LDS: thrl_sampled_chain's working set, V (8 Jn), 2 Jn bytes per QTable
 * agent (its node entries), and per neural agent two tile buffers of 4 (THRL_SPN_TILE A_i + 3) bytes: the node rows
 * (4 Jn A_i bytes) are streamed through them in ascending j and Zn(j) is recomputed from the resident tile, not kept:
 *   thrl_sampled_chain's sum + r16(8 Jn) + sum of r16(2 Jn) (QTable i) + sum of 2 r16(4 (64 A_i + 3)) (neural i)
 * Above THRL_SP_MAX_LDS or the device's own limit the call returns THRL_ERR_UNSUPPORTED without launching.  QTable 21 x
 * Reinforce 21 at Jn = 1,121 takes 79,232 bytes (two blocks per 160 KB CU); against a 32-action network at Jn = 1,121 a
 * QTable of 27 actions (T = 864, D = 724, 153,696 bytes) fits and one of 28 (T = D = 896, 179,728 bytes) does not.
 *
 * Returns as thrl_sampled_chain, and THRL_ERR_BAD_CONFIG for n_nodes < 2, band_w < 1, a scalar noise_prob outside
 * [0, 1] or NaN, or both start flags; THRL_ERR_UNSUPPORTED for n_nodes > THRL_STAT_MAX_CELLS or the working set;
 * THRL_ERR_NULL for a missing nprob[i] of a neural agent, npolicy, band_lo, band, noise_price, noise_reward or node_w.
 * Everything is decided from the shape before any pointer is dereferenced.
 */
#define THRL_SPN_START_TUPLE 1
#define THRL_SPN_START_RESET 2
#define THRL_SPN_TILE 64
typedef struct {
    int32_t n_games;                 /* G >= 1                                           */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t n_nodes;                 /* Jn in [2, THRL_STAT_MAX_CELLS]                   */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t max_iters;               /* in [1, THRL_STAT_MAX_ITERS]                      */
    int32_t flags;                   /* THRL_SPN_START_TUPLE or THRL_SPN_START_RESET     */
    int32_t reserved;                /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  tol;                     /* >= 0                                             */
    double  noise_prob;              /* in [0, 1], read when noise_prob_g is NULL        */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const int32_t* start;            /* device [G], with THRL_SPN_START_TUPLE            */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const float* nprob[THRL_MAXA];   /* device [G][Jn][A_i] for the neural agents        */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const uint16_t* npolicy;         /* device [G][N][Jn]                                */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* price;             /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_price;       /* device [T]                                       */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* node_w;            /* device [Jn]                                      */
    int32_t* iters;                  /* device [G]                                       */
    double*  change;                 /* device [G]                                       */
    double*  mass;                   /* device [G]                                       */
    double*  samp_reward;            /* device [N][G]                                    */
    double*  samp_action;            /* device [N][G]                                    */
    double*  samp_price;             /* device [G]                                       */
    double*  agree;                  /* device [G]                                       */
    double*  pi;                     /* device [G][T] or NULL                            */
    double*  max_jump;               /* device [G] or NULL                               */
} thrl_sampled_noise_chain_args;
int thrl_sampled_noise_chain(const thrl_cfg* cfg, const thrl_sampled_noise_chain_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* THRL_H */
