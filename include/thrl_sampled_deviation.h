/*
 * thrl_sampled_deviation.h -- the deviation test of sampled play, an analysis call of libthrl_hip.so added after
 * include/thrl.h's set was closed at ABI version 4.  Additive: THRL_ABI_VERSION stays 4, and a program that includes only
 * thrl.h sees what it saw.
 */
#ifndef THRL_SAMPLED_DEVIATION_H
#define THRL_SAMPLED_DEVIATION_H

#include "thrl.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * thrl_sampled_deviation: the DEVIATION TEST of SAMPLED play -- the expected impulse response of the agents' stochastic
 * policies to a forced deviation of one of them.  thrl_sampled_chain says what the stochastic policies earn in the long
 * run, thrl_sampled_response what each agent gives up against rivals that sample; this call asks the question that
 * separates collusion from failure to learn: if one agent departs from its policy for a few periods, do the others'
 * sampled policies punish it, how deep is the punishment, how long until play is back, and was the departure
 * profitable?  No reference counterpart.  Noise-free play; under demand noise the call is thrl_sampled_deviation_noise
 * (include/thrl_sampled_deviation_noise.h).  No episodes are sampled: the tuple played is a Markov
 * chain on the T action tuples whose row depends on the tuple only through its price, and the call propagates a
 * distribution through that chain, L periods with the deviator's policy replaced, then K - L plain periods, and records
 * what every period's distribution earns.  Of a valid cfg only n_agents and n_actions are used (cfg.gamma is not read);
 * nothing of a batch is read or written, every input is read only.
 *
 * Notation, the per-config tables (grp_first, grp_perm, reward, scaled, price), prob, dpolicy, eps / eps_g, P_i(k|d),
 * S_i(d), Z(d), M(d), W(d) and the clamps are thrl_sampled_chain's (include/thrl.h).  All arithmetic is float64.  Every
 * operation is rounded once, with no contraction.  Every sum runs in ascending index from 0.0, in the order written.
 *
 * Deviator and deviation strategy.  The deviator is delta = args.deviator, with A = A_delta actions.  While the
 * deviation lasts, the deviator plays a deterministic strategy ad_g(d) of the price row d: an agent conditions on the
 * price alone.  Three modes:
 *   dev_action in [0, A)   ad_g(d) = dev_action at every price
 *   dev_action = -1        the one-period best response to the rivals' mixed policies at that price: ad_g(d) is the first
 *                          maximum under strict > over k of
 *                            q(d, k) = (sum over the t with a_delta(t) = k, ascending t, of w(t|d) * reward_delta(t))
 *                                      / Z_-delta(d)
 *                          with w(t|d) and Z_-delta(d) as in include/thrl_response.h: the product over j != delta,
 *                          ascending j, the first factor taken as is (thrl_sampled_response's Q_V with V = 0)
 *   flag THRL_SD_POLICY    ad_g(d) = min(dev_policy[g][d], A - 1), dev_policy device uint16 [G][D]: e.g. one agent's
 *                          slice of thrl_sampled_response's br_policy, the patient best reply.  dev_action must be -1
 *
 * The deviation step is thrl_sampled_chain's step without the lazy half, with the deviator's row replaced:
 * P_delta(k|d) = 1.0 for k = ad_g(d), else 0.0, and S_delta(d) = 1.0 exactly; Z is recomputed with these values (the
 * deviator is then a QTable agent with hi = 1.0, lo = 0.0 and greedy row ad_g).  The plain step uses the agents' own
 * rows.  In both
 *   M(d)   = sum over the t with row(t) = d of x(t)          ascending t from 0.0
 *   W(d)   = M(d) / Z(d)
 *   x'(t') = sum_d ((W(d) * P_0(a_0(t')|d)) * P_1(a_1(t')|d)) * ...      ascending d from 0.0; a d with W(d) == 0.0 is
 *            skipped
 *
 * Propagation.  x_0 = weights[g] (device double [G][T], required), e.g. thrl_sampled_chain's pi.  For tau = 0 .. K - 1:
 * x_{tau+1} = step_tau(x_tau), the deviation step for tau < L and the plain step otherwise.  x_tau is the distribution of
 * the tuple played one period before tau, whose price the agents see at tau; x_{tau+1} is the distribution of the tuple
 * played in period tau.
 *
 * Outputs, per game:
 *   base_reward[i][g] = sum_t x_0(t) * reward_i(t),  base_action[i][g] the same with scaled_i,  base_price[g] with price:
 *                       with thrl_sampled_chain's pi as weights bit for bit its samp_reward, samp_action and samp_price
 *   dev_share[g]      = sum_d M_0(d) * (1.0 - P_delta(ad_g(d)|d) / S_delta(d)), with the deviator's own row and M_0 from
 *                       x_0 (divide, subtract, multiply, add): the share of periods the deviation changes.  Exactly 0.0
 *                       when a QTable deviator at eps 0 is "deviated" to its own greedy row
 *   the outcome of period tau: r_i(tau), the scaled action and the price are the baseline's sums over x_{tau+1};
 *                       dist(tau) = 0.5 * sum_t |x_{tau+1}(t) - x_0(t)|;  diff(tau) = r_delta(tau) - base_reward_delta
 *   gain[g]           = sum_tau w_tau * diff(tau), w_0 = 1, w_{tau+1} = w_tau * gamma (subtract, multiply, add); gamma =
 *                       sweep_gamma[delta][g] (device double [N][G]) if given, else args.gamma; a host-visible value
 *                       outside [0, 1] (NaN included) is THRL_ERR_BAD_CONFIG
 *   gain_dev[g]       = the same sum over tau < L
 *   low[g], low_step[g]   the first minimum of diff(tau) over tau >= L; 0.0 and -1 when L = K
 *   ret_step[g]       = the first tau >= L with dist(tau) <= ret_tol, else -1
 *   dist[g] = dist(K - 1),  mass[g] = sum_t x_K(t)
 * Optional rows for tau in [row_begin, row_begin + row_count): reward_rows and action_rows [row_count][N][G] hold r_i(tau)
 * and the scaled action, price_rows and dist_rows [row_count][G] the price and dist(tau): the shapes
 * thrl_tuple_deviation_noise writes, so thrl_group_stats reduces them as they are.  The kernel walks all K periods
 * whatever rows it stores.
 * A game whose eps_g entry for a QTable agent lies outside [0, 1] (NaN included) is device data: it gets zeros in every
 * float64 output, low_step = ret_step = -1, and zeros in its rows.  No other game is affected.
 *
 * Working set.  A game is solved by one 256-thread block in LDS: thrl_sampled_chain's working set, ad_g (2 D), the
 * deviation step's Z (8 D) and one more staging row (512 bytes) for the distance, each array rounded up to 16 bytes:
 *   thrl_sampled_chain's sum + r16(2 D) + r16(8 D) + 512
 * q(d, k) needs no array of its own: reward_delta is staged in the second iterate, which is dead until the first step.
 * The call returns THRL_ERR_UNSUPPORTED, without launching, when the sum exceeds THRL_SD_MAX_LDS = 160 KB (a CU's LDS on
 * gfx950) or the device's own limit.  QTable 21 x Reinforce 21 (T = D = 441) takes 62,160 bytes.
 *
 * Cost.  A period is one non-lazy chain step, T D N multiplications, and T (2 N + 2) for its sums; the best response adds
 * D T (N - 1) once per game.
 *
 * Returns THRL_ERR_BAD_CONFIG for n_games < 1, an unknown flag, a reserved word != 0, a kind outside [0, 3], a neural
 * agent with actions outside [2, 32], n_tuples < 1 or n_tuples != prod_i n_actions_i, n_prices outside [1, n_tuples], a
 * deviator outside [0, N), dev_len < 1, n_steps < dev_len or > THRL_DEV_MAX_STEPS, dev_action outside {-1} + [0, A) (with
 * THRL_SD_POLICY: other than -1), a row range outside [0, n_steps), ret_tol < 0 or NaN, gamma or eps as above;
 * THRL_ERR_UNSUPPORTED for a CAC agent (kind 3), n_tuples > THRL_TP_MAX_TUPLES or the working set; THRL_ERR_NULL for a
 * missing cfg, args, prob[i] of a neural agent, dpolicy, table (grp_first, grp_perm, reward, scaled, price), weights,
 * dev_policy with THRL_SD_POLICY, or per-game output.  All of these are decided before any launch, the host-visible
 * arguments and the working set before any pointer is looked at.
 */
#define THRL_SD_POLICY 1
#define THRL_SD_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of prob and dpolicy                */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t deviator;                /* delta in [0, N)                                  */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K in [L, THRL_DEV_MAX_STEPS]                     */
    int32_t dev_action;              /* fixed action index of delta, or -1               */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t flags;                   /* THRL_SD_POLICY                                   */
    int32_t reserved[2];             /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  gamma;                   /* in [0, 1], read when sweep_gamma is NULL         */
    double  ret_tol;                 /* >= 0                                             */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const uint16_t* dev_policy;      /* device [G][D], with THRL_SD_POLICY               */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* price;             /* device [T]                                       */
    const double* weights;           /* device [G][T] (required): x_0                    */
    double*  base_reward;            /* device [N][G]                                    */
    double*  base_action;            /* device [N][G]                                    */
    double*  base_price;             /* device [G]                                       */
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
    double*  price_rows;             /* device [row_count][G] or NULL                    */
    double*  dist_rows;              /* device [row_count][G] or NULL                    */
} thrl_sampled_deviation_args;
int thrl_sampled_deviation(const thrl_cfg* cfg, const thrl_sampled_deviation_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THRL_SAMPLED_DEVIATION_H */
