/*
 * thrl_response_noise.h -- thrl_sampled_response's twin under demand noise.  Additive like include/thrl_response.h, which
 * it includes: THRL_ABI_VERSION stays 4, and a program that includes only thrl.h or thrl_response.h sees what it saw.
 */
#ifndef THRL_RESPONSE_NOISE_H
#define THRL_RESPONSE_NOISE_H

#include "thrl_response.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * thrl_sampled_response_noise: exact BEST RESPONSES to the rivals' STOCHASTIC policies UNDER DEMAND NOISE, the
 * environment the reference ships (NoisyPriceState, noise_prob = 0.05): thrl_sampled_response's question -- is each
 * stochastic policy a good reply to the others? -- in the environment of thrl_sampled_noise_chain.  No reference
 * counterpart.  Of a valid cfg only n_agents and n_actions are used (cfg.gamma is not read); nothing of a batch is read
 * or written, every input is read only.
 *
 * Notation is thrl_sampled_noise_chain's (include/thrl.h) and thrl_sampled_response's (include/thrl_response.h): G, T, D,
 * a_i(t), row(t) (grp_first, grp_perm, clamped when staged), reward, noise_reward (device double [N][T]); Jn =
 * args.n_nodes in [2, THRL_STAT_MAX_CELLS], W = args.band_w >= 1, nn(t, j) = band[t][j - band_lo[t]] for band_lo[t] <= j <
 * band_lo[t] + W, else 0 (any band_lo is safe); prob[i], dpolicy, nprob[i] (device float32 [G][Jn][A_i]), npolicy (device
 * uint16 [G][N][Jn], clamped to A_i - 1), eps / eps_g; P_i(k|d), S_i(d) on the rows at the distinct prices, Pn_i(k|j),
 * Sn_i(j) the same definitions on the node rows.  p = args.noise_prob_g[g] (device double [G]) if given, else
 * args.noise_prob; q = 1 - p.  gamma by thrl_sampled_response's rule (sweep_gamma, else gamma[i]).  All arithmetic is
 * float64, every operation is rounded once (no contraction), every sum runs in ascending index from 0.0, in the order
 * written here.
 *
 * States.  An agent sees the price, so its problem has S = D + Jn states: state s < D is the distinct price d = s,
 * reached with probability q after a tuple; state s = D + j is node j of the redrawn price.  Node 0, the atom at price 0,
 * is a state like any other (only its node_w is 0, which this call does not read).  A value function V has two parts,
 * V_D [D] and V_N [Jn].  At a price-state the rows P, S, Z_-i come from prob / dpolicy, at a node-state from nprob /
 * npolicy, by the same definitions: P_i(k|s), S_i(s), Z_-i(s).
 *   Rn(t)    = q * reward_i(t) + p * noise_reward_i(t)
 *   b_V(t)   = sum over w = 0 .. W - 1, ascending, from 0.0, of band[t][w] * V_N[band_lo[t] + w]; nodes outside [0, Jn) are
 *              skipped
 *   z_V(t)   = q * V_D[row(t)] + p * b_V(t)
 *   U_V(t)   = Rn(t) + gamma * z_V(t)
 *   w(t|s)   = the product over j != i, ascending j, of P_j(a_j(t)|s); the first factor is taken as is (N = 1: 1.0)
 *   Q_V(s,k) = (sum over the t with a_i(t) = k, ascending t, of w(t|s) * U_V(t)) / Z_-i(s)
 *
 * Solver.  V_pi, V*, sigma*, the margin, the modal start, the caps and loss(s) are thrl_sampled_response's, word for
 * word, with the index s over the S states in place of d; chg is the maximum over all S states; U_V is computed once per
 * tuple per sweep.
 *
 * Outputs, per selected agent i and game g (device [N][G]; the entries of other agents are not written):
 *   iters, sweeps       as in thrl_sampled_response
 *   n_diff_prices       the price-states where sigma*(s) differs from the modal action;  n_diff_nodes: the node-states
 *   loss_all            max_s loss(s) over all S states
 *   loss_prices_mean    (sum of loss(s) over the price-states) / D;   loss_nodes_mean: (sum over the node-states) / Jn
 * and with args.pi (device double [G][T], thrl_sampled_noise_chain's pi), M(d) as in thrl_sampled_response and
 *   nu(j)    = sum over ascending t of pi(t) * nn(t, j)         (zero terms change nothing)
 *   w(d)     = q * M(d),   w(D + j) = p * nu(j)
 * the long-run distribution of the state in which a decision is made (the weights add up to one in exact arithmetic):
 * loss_w, gain_w, v_w, br_prob_w are thrl_sampled_response's terms with w(s) in place of M(d), each one sum from 0.0 over
 * the price-states, then the node-states.  exploit = (1 - gamma_i) * gain_w stays in reward units per period.
 * Optional, device [N][G][S], price-states first: br_policy (uint16) = sigma*, v_opt = V*, v_pi = V_pi.
 *
 * Unsolved games.  An entry of noise_prob_g outside (0, 1] (NaN included) or a bad entry of eps_g refuses the game
 * (every selected agent of it): iters = -1, zeros in every output, br_policy = 0.  An (agent, game) with gamma outside
 * [0, 1) (NaN included), or capped: iters = -1, sweeps = the sweeps made, n_diff_* = 0, NaN in every float output,
 * br_policy = the modal action.  No other (agent, game) is affected.  A host-visible noise_prob outside (0, 1] is
 * THRL_ERR_BAD_CONFIG: p = 0 is thrl_sampled_response's job.
 *
 * Working set.  A game is solved by one 256-thread block in LDS: V, V', V_pi, Z_-i and S_i over the states (8 S each), U
 * and Rn (8 T each), the rows at the distinct prices as in thrl_sampled_chain (4 D A_j per network, 2 D per QTable agent),
 * the grouping (2 (D + 1) + 2 T), row(t) (2 T), sigma and the modal action (2 S each), a QTable agent's node entries
 * (2 Jn each), 2,048 bytes for the block's maxima and 256 bytes of per-game constants; each array rounded up to 16 bytes:
 *   5 r16(8 S) + 2 r16(8 T) + sum_j (QTable: r16(2 D); network: r16(4 D A_j)) + r16(2 (D + 1)) + 2 r16(2 T) + 2 r16(2 S)
 *   + sum over the QTable agents of r16(2 Jn) + 2,048 + 256
 * The networks' node rows (4 Jn A_j bytes each: 94 KB for 21 actions at Jn = 1,121) are not part of it: they are read
 * from global memory every sweep, and so is band.  The call returns THRL_ERR_UNSUPPORTED, without launching and before
 * any pointer is read, when the sum exceeds THRL_SRN_MAX_LDS = 160 KB (a CU's LDS on gfx950) or the device's own limit.
 * QTable 21 x Reinforce 21 (T = D = 441) at Jn = 1,121 takes 121,024 bytes.  The refusal's message is the shared one of the
 * calls that plan a working set, "... bytes of LDS per game (N=.., n_cells=..)": n_cells there is S = D + Jn, the states.
 *
 * Cost.  A sweep of a deterministic strategy is S T / A_i + T W multiply-adds against thrl_sampled_response's D T / A_i
 * (two agents), a sweep of the mixed policy or an improvement step S T + T W against D T.
 *
 * Returns as thrl_sampled_response, and THRL_ERR_BAD_CONFIG for n_nodes < 2, band_w < 1 or a scalar noise_prob outside
 * (0, 1]; THRL_ERR_UNSUPPORTED for n_nodes > THRL_STAT_MAX_CELLS or the working set; THRL_ERR_NULL for a missing nprob[i]
 * of a neural agent, npolicy, band_lo, band, noise_reward, n_diff_prices, n_diff_nodes, loss_prices_mean or
 * loss_nodes_mean.
 */
#define THRL_SRN_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of prob, nprob, dpolicy and npolicy */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t n_nodes;                 /* Jn in [2, THRL_STAT_MAX_CELLS]                   */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t agents;                  /* bit i: solve agent i; non-empty, bits < N        */
    int32_t max_sweeps;              /* in [1, THRL_STAT_MAX_ITERS], per evaluation      */
    int32_t flags;                   /* 0                                                */
    int32_t reserved[2];             /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  gamma[THRL_MAXA];        /* in [0, 1), read when sweep_gamma is NULL         */
    double  eval_tol;                /* >= 0                                             */
    double  noise_prob;              /* in (0, 1], read when noise_prob_g is NULL        */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const float* nprob[THRL_MAXA];   /* device [G][Jn][A_i] for the neural agents        */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const uint16_t* npolicy;         /* device [G][N][Jn]                                */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_reward;      /* device [N][T]                                    */
    const double* pi;                /* device [G][T] or NULL                            */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* sweeps;                 /* device [N][G]                                    */
    int32_t* n_diff_prices;          /* device [N][G]                                    */
    int32_t* n_diff_nodes;           /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_prices_mean;       /* device [N][G]                                    */
    double*  loss_nodes_mean;        /* device [N][G]                                    */
    double*  loss_w;                 /* device [N][G], with pi                           */
    double*  gain_w;                 /* device [N][G], with pi                           */
    double*  v_w;                    /* device [N][G], with pi                           */
    double*  br_prob_w;              /* device [N][G], with pi                           */
    uint16_t* br_policy;             /* device [N][G][D + Jn] or NULL                    */
    double*  v_opt;                  /* device [N][G][D + Jn] or NULL                    */
    double*  v_pi;                   /* device [N][G][D + Jn] or NULL                    */
} thrl_sampled_response_noise_args;
int thrl_sampled_response_noise(const thrl_cfg* cfg, const thrl_sampled_response_noise_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THRL_RESPONSE_NOISE_H */
