/*
 * thrl_response.h -- the analysis calls of libthrl_hip.so added after include/thrl.h's set was closed at ABI version 4.
 * Additive: THRL_ABI_VERSION stays 4, and a program that includes only thrl.h sees what it saw.
 */
#ifndef THRL_RESPONSE_H
#define THRL_RESPONSE_H

#include "thrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * thrl_sampled_response: exact BEST RESPONSES to the rivals' STOCHASTIC policies -- the exploitability of sampled play.
 * thrl_sampled_chain says what the stochastic policies earn in the long run; this call says whether each of them is a
 * good reply to the others: for every selected agent i the value V_pi of its own mixed policy against the sampling
 * rivals, the value V* and the strategy sigma* of its best deterministic reply, and what it gives up.  No reference
 * counterpart.  Noise-free play only.  Of a valid cfg only n_agents and n_actions are used (cfg.gamma is not read);
 * nothing of a batch is read or written, every input is read only.
 *
 * Notation is thrl_sampled_chain's (include/thrl.h): G = args.n_games >= 1, T = args.n_tuples = prod_i n_actions_i <=
 * THRL_TP_MAX_TUPLES, D = args.n_prices in [1, T]; a_i(t) = (t / tstride_i) mod A_i; row(t), the index of price(t) among
 * the distinct prices, given as grp_first (device int32 [D + 1]) and grp_perm (device int32 [T]), clamped when staged;
 * reward (device double [N][T]).  prob[i] (device float32 [G][D][A_i]) for the neural agents, dpolicy (device uint16
 * [G][N][D], clamped to A_i - 1) and eps / eps_g exactly as there, and so are
 *   P_j(k|d), S_j(d)      the float32 network rows widened and their ascending sum from 0.0; for a QTable agent
 *                         lo = eps / A_j, hi = (1 - eps) + lo, P_j(k|d) = hi for k = g_j(d) else lo, S_j(d) = 1.0 exactly
 * A scalar eps outside [0, 1] (NaN included) for a QTable agent is THRL_ERR_BAD_CONFIG; such an entry of eps_g is device
 * data and refuses that game only (every selected agent of it): iters = -1, zeros in every output, br_policy = 0.
 * All arithmetic is float64, every operation is rounded once (no contraction), every sum runs in ascending index from
 * 0.0, in the order written here.
 *
 * An agent conditions on the price alone, so agent i's problem against the rivals' stochastic policies lives on the D
 * distinct prices.  gamma = args.sweep_gamma[i][g] (device double [N][G]) if given, else args.gamma[i]; a host-visible
 * gamma[i] of a selected agent outside [0, 1) is THRL_ERR_BAD_CONFIG, an entry of sweep_gamma outside it is device data:
 * that (agent, game) is not solved (below).  For a value function V on the prices:
 *   U_V(t)    = reward_i(t) + gamma * V(row(t))
 *   w(t|d)    = the product over j != i, ascending j, of P_j(a_j(t)|d); the first factor is taken as is (N = 1: 1.0)
 *   Z_-i(d)   = the same product of the S_j(d)
 *   Q_V(d, k) = (sum over the t with a_i(t) = k, ascending t, of w(t|d) * U_V(t)) / Z_-i(d)
 *
 * V_pi, the value of the agent's own mixed policy: Jacobi sweeps from V = 0,
 *   V'(d) = (sum over k ascending of P_i(k|d) * Q_V(d, k)) / S_i(d),     chg = max_d |V'(d) - V(d)|
 * stop after the first sweep with chg <= args.eval_tol; after args.max_sweeps sweeps without it the (agent, game) is
 * CAPPED.
 *
 * V* and sigma*: thrl_tuple_equilibrium_noise's solver over the D prices.  Policy iteration over deterministic
 * strategies from sigma_0(d) = the agent's modal action: the first maximum of P_i(.|d) under strict >, for a QTable agent
 * g_i(d).  Round n = 0, 1, ..: V_n = the evaluation of sigma_n by Jacobi sweeps V'(d) = Q_V(d, sigma_n(d)) with the same
 * stopping rule and cap (per evaluation), warm-started from V_{n-1} (round 0: from V_pi); if n == THRL_EQ_MAX_ITERS the
 * (agent, game) is capped; with margin = ((2 gamma) gamma) eval_tol / (1 - gamma): ba(d) = the first maximum of
 * Q_{V_n}(d, .) under strict >; sigma_{n+1}(d) = ba(d) if Q(d, ba(d)) > Q(d, sigma_n(d)) + margin, else sigma_n(d) (the
 * incumbent is kept); if no price changed: iters = n, V* = V_n, sigma* = sigma_n, stop.
 *   loss(d) = 0 if V*(d) == V_pi(d) or V*(d) == 0, else (V*(d) - V_pi(d)) / V*(d)
 *
 * Outputs, per selected agent i and game g (device [N][G]; the entries of other agents are not written):
 *   iters        the rounds; -1 = not solved
 *   sweeps       all sweeps, the V_pi evaluation included
 *   n_diff       the prices where sigma*(d) differs from the modal action
 *   loss_all     max_d loss(d)
 *   loss_mean    (sum_d loss(d)) / D
 * and with args.pi (device double [G][T], thrl_sampled_chain's pi) and M(d) = the sum of pi(t) over the t with row(t) =
 * d in ascending t (thrl_sampled_chain's M):
 *   loss_w       sum_d M(d) * loss(d)
 *   gain_w       sum_d M(d) * (V*(d) - V_pi(d))
 *   v_w          sum_d M(d) * V_pi(d)
 *   br_prob_w    sum_d (M(d) * P_i(sigma*(d)|d)) / S_i(d): the long-run share of steps on which the agent already plays
 *                its best response
 * Optional, device [N][G][D]: br_policy (uint16) = sigma*, v_opt = V*, v_pi = V_pi.
 * An (agent, game) with gamma outside [0, 1) (NaN included), or capped: iters = -1, sweeps = the sweeps made, n_diff = 0,
 * NaN in every float output, br_policy = the modal action.  No other (agent, game) is affected.
 *
 * Working set.  A game is solved by one 256-thread block in LDS: V, V', V_pi, Z_-i and S_i (8 D each), U and reward_i
 * (8 T each), the rows as in thrl_sampled_chain (4 D A_j per network, 2 D per QTable agent), the grouping (2 (D + 1) +
 * 2 T), row(t) (2 T), sigma and the modal action (2 D each), 2,048 bytes for the block's maxima, 256 bytes of per-game
 * constants and, where 2 D <= 256 and 8 D max_j A_j <= 32,768, the latter bytes for the Q_V(d, k) a team of threads
 * shares per price; each array rounded up to 16 bytes.  The call returns THRL_ERR_UNSUPPORTED, without launching, when
 * the sum exceeds THRL_SR_MAX_LDS = 160 KB (a CU's LDS on gfx950) or the device's own limit.  QTable 21 x Reinforce 21
 * (T = D = 441) takes 69,488 bytes.
 *
 * Cost.  A sweep of the mixed policy or an improvement step is D T (N - 1) multiply-adds, a sweep of a deterministic
 * strategy 1 / A_i of that; the sweeps to eval_tol grow like ln(eval_tol) / ln(gamma).
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, flags != 0, a reserved word != 0, agents == 0 or with a bit >= N, a kind
 * outside [0, 3], a neural agent with actions outside [2, 32], n_tuples < 1 or n_tuples != prod_i n_actions_i, n_prices
 * outside [1, n_tuples], gamma or eps as above, max_sweeps outside [1, THRL_STAT_MAX_ITERS], eval_tol < 0 or NaN;
 * THRL_ERR_UNSUPPORTED for a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES or the working set; THRL_ERR_NULL for a
 * missing cfg, args, prob[i] of a neural agent, dpolicy, grp_first, grp_perm, reward, iters, sweeps, n_diff, loss_all,
 * loss_mean, or with pi loss_w, gain_w, v_w, br_prob_w.
 */
#define THRL_SR_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of prob and dpolicy                */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t agents;                  /* bit i: solve agent i; non-empty, bits < N        */
    int32_t max_sweeps;              /* in [1, THRL_STAT_MAX_ITERS], per evaluation      */
    int32_t flags;                   /* 0                                                */
    int32_t reserved[2];             /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  gamma[THRL_MAXA];        /* in [0, 1), read when sweep_gamma is NULL         */
    double  eval_tol;                /* >= 0                                             */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* pi;                /* device [G][T] or NULL                            */
    int32_t* iters;                  /* device [N][G]                                    */
    int32_t* sweeps;                 /* device [N][G]                                    */
    int32_t* n_diff;                 /* device [N][G]                                    */
    double*  loss_all;               /* device [N][G]                                    */
    double*  loss_mean;              /* device [N][G]                                    */
    double*  loss_w;                 /* device [N][G], with pi                           */
    double*  gain_w;                 /* device [N][G], with pi                           */
    double*  v_w;                    /* device [N][G], with pi                           */
    double*  br_prob_w;              /* device [N][G], with pi                           */
    uint16_t* br_policy;             /* device [N][G][D] or NULL                         */
    double*  v_opt;                  /* device [N][G][D] or NULL                         */
    double*  v_pi;                   /* device [N][G][D] or NULL                         */
} thrl_sampled_response_args;
int thrl_sampled_response(const thrl_cfg* cfg, const thrl_sampled_response_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THRL_RESPONSE_H */
