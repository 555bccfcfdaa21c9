/*
 * thrl_sampled_deviation_noise.h -- thrl_sampled_deviation's twin under demand noise.  Additive like
 * include/thrl_sampled_deviation.h, which it includes: THRL_ABI_VERSION stays 4, and a program that includes only thrl.h
 * or thrl_sampled_deviation.h sees what it saw.
 */
#ifndef THRL_SAMPLED_DEVIATION_NOISE_H
#define THRL_SAMPLED_DEVIATION_NOISE_H

#include "thrl_response_noise.h"
#include "thrl_sampled_deviation.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * thrl_sampled_deviation_noise: the DEVIATION TEST of SAMPLED play UNDER DEMAND NOISE, the environment the reference
 * ships (NoisyPriceState, noise_prob = 0.05): thrl_sampled_deviation's question -- if one agent departs from its policy
 * for a few periods, do the others' sampled policies punish it, how deep, how long until play is back, and did it pay? --
 * in the environment of thrl_sampled_noise_chain.  No reference counterpart.  No episodes are sampled: the call
 * propagates a distribution over the tuple played through thrl_sampled_noise_chain's chain without the lazy half, L
 * periods with the deviator's policy replaced, then K - L plain periods, and records what every period's distribution
 * earns in expectation over the redrawn demand.  Of a valid cfg only n_agents and n_actions are used (cfg.gamma is not
 * read); nothing of a batch is read or written, every input is read only.
 *
 * Notation is thrl_sampled_noise_chain's (include/thrl.h), thrl_sampled_deviation's (include/thrl_sampled_deviation.h)
 * and thrl_sampled_response_noise's (include/thrl_response_noise.h): G, T, D, a_i(t), row(t) (grp_first, grp_perm, clamped
 * when staged), reward, scaled, price, noise_reward, noise_price; Jn = args.n_nodes in [2, THRL_STAT_MAX_CELLS], W =
 * args.band_w >= 1, nn(t, j) = band[t][j - band_lo[t]] for band_lo[t] <= j < band_lo[t] + W, else 0 (any band_lo is
 * safe); prob[i], dpolicy, nprob[i] (device float32 [G][Jn][A_i]), npolicy (device uint16 [G][N][Jn], clamped to
 * A_i - 1), eps / eps_g; P_i(k|d), S_i(d), Z(d) on the rows at the distinct prices, Pn_i(k|j), Sn_i(j), Zn(j) the same
 * definitions on the node rows.  Per game p = args.noise_prob_g[g] (device double [G]) if given, else args.noise_prob;
 * q = 1 - p.  All arithmetic is float64.  Every operation is rounded once, with no contraction.  Every sum runs in
 * ascending index from 0.0, in the order written.
 *
 * States and the deviation strategy.  The deviator delta = args.deviator, with A = A_delta actions, conditions on the
 * price, so its strategy lives on S = D + Jn states: the D distinct prices first, then the Jn nodes of a redrawn price --
 * thrl_sampled_response_noise's order, so one agent's slice of its br_policy can be passed as it is.  At a price-state
 * s = d the rows P, S come from prob / dpolicy, at a node-state s = D + j from nprob / npolicy, by the same definitions:
 * P_i(k|s), S_i(s).  ad_g(s) takes one of three forms:
 *   dev_action in [0, A)   ad_g(s) = dev_action at every state
 *   dev_action = -1        the one-period best response at state s: the first maximum under strict > over k of
 *                            (sum over the t with a_delta(t) = k, ascending t, of w(t|s) * Rn_delta(t)) / Z_-delta(s)
 *                          with Rn_i(t) = q * reward_i(t) + p * noise_reward_i(t) (two products, one add) and w(t|s),
 *                          Z_-delta(s) as in include/thrl_response_noise.h: the products over j != delta, ascending j, of
 *                          P_j(a_j(t)|s) and of S_j(s), the first factor taken as is (that header's Q_V with V = 0)
 *   flag THRL_SDN_POLICY   ad_g(s) = min(dev_policy[g][s], A - 1), dev_policy device uint16 [G][D + Jn].  dev_action
 *                          must be -1
 *
 * Steps.  The deviation step replaces the deviator's row at the prices AND at the nodes: P_delta(k|s) = 1.0 for
 * k = ad_g(s), else 0.0, and S_delta(s) = 1.0 exactly; Z(d) and Zn(j) are recomputed with these values.  The plain step
 * uses the agents' own rows.  Both are thrl_sampled_noise_chain's step without the lazy half, with the step's rows:
 *   M(d)   = sum over the t with row(t) = d of x(t)         ascending t from 0.0;   W(d) = M(d) / Z(d)
 *   nu(j)  = sum_t x(t) * nn(t, j)                          ascending t from 0.0 (zero terms change nothing);
 *   V(j)   = nu(j) / Zn(j)
 *   Sd(t') = sum_d ((W(d) * P_0(a_0(t')|d)) * P_1(a_1(t')|d)) * ...      ascending d, a d with W(d) == 0.0 skipped
 *   Sn(t') = sum_j ((V(j) * Pn_0(a_0(t')|j)) * Pn_1(a_1(t')|j)) * ...    ascending j, a j with V(j) == 0.0 skipped
 *   x'(t') = q * Sd(t') + p * Sn(t')                        two products, one add
 *
 * Propagation.  x_0 = weights[g] (device double [G][T], required), e.g. thrl_sampled_noise_chain's pi.  For tau = 0 ..
 * K - 1: x_{tau+1} = step_tau(x_tau), the deviation step for tau < L and the plain step otherwise.
 *
 * Outputs, per game: thrl_sampled_deviation's, with the noisy expectations.
 *   base_reward[i][g] = sum_t x_0(t) * (q * reward_i(t) + p * noise_reward_i(t)),  base_action[i][g] = sum_t x_0(t) *
 *                       scaled_i(t),  base_price[g] = sum_t x_0(t) * (q * price(t) + p * noise_price(t)): with
 *                       thrl_sampled_noise_chain's pi as weights bit for bit its samp_reward, samp_action and samp_price
 *   dev_share[g]      = q * (sum_d M_0(d) * (1.0 - P_delta(ad_g(d)|d) / S_delta(d)))
 *                       + p * (sum_j nu_0(j) * (1.0 - Pn_delta(ad_g(D + j)|j) / Sn_delta(j))), with the deviator's OWN rows
 *                       and M_0, nu_0 from x_0 (per term: divide, subtract, multiply, add)
 *   the outcome of period tau: r_i(tau), the scaled action and the price are the baseline's sums over x_{tau+1};
 *                       dist(tau) = 0.5 * sum_t |x_{tau+1}(t) - x_0(t)|;  diff(tau) = r_delta(tau) - base_reward_delta
 *   gain, gain_dev, low, low_step, ret_step, dist, mass, the optional rows for tau in [row_begin, row_begin + row_count),
 *                       the gamma rule (sweep_gamma[delta][g] if given, else args.gamma, a host-visible value outside
 *                       [0, 1] THRL_ERR_BAD_CONFIG) are thrl_sampled_deviation's, word for word
 *
 * The rule for p = 0.  p in [0, 1] is allowed, zero included, as in thrl_sampled_noise_chain.  With p = 0, q * Sd + p * Sn
 * = Sd exactly, Rn = reward exactly, and the price-states' best response is thrl_sampled_deviation's: every output and
 * row then has the bits of thrl_sampled_deviation on the same inputs (dev_policy's first D entries per game).
 *
 * Unsolved games.  A game whose eps_g entry for a QTable agent, or whose noise_prob_g entry, lies outside [0, 1] (NaN
 * included) is device data: it gets zeros in every float64 output, low_step = ret_step = -1, and zeros in its rows.  No
 * other game is affected.
 *
 * Working set.  A game is solved by one 256-thread block in LDS: thrl_sampled_noise_chain's working set, ad_g over the
 * states (2 (D + Jn)), the deviation step's Z (8 D) and one more staging row (512 bytes) for the distance, each array
 * rounded up to 16 bytes:
 *   thrl_sampled_noise_chain's sum + r16(2 (D + Jn)) + r16(8 D) + 512
 * The best response needs no array of its own: Rn_delta is staged in the second iterate, which is dead until the first
 * step, and dev_share's node terms replace nu_0.  The networks' node rows are streamed as in thrl_sampled_noise_chain; a
 * network deviator's are not read while the deviation lasts.  The call returns THRL_ERR_UNSUPPORTED, without launching,
 * when the sum exceeds THRL_SDN_MAX_LDS = 160 KB (a CU's LDS on gfx950) or the device's own limit.  QTable 21 x
 * Reinforce 21 (T = D = 441) at Jn = 1,121 takes 86,416 bytes: one block per CU.
 *
 * Cost.  A period is one non-lazy step of thrl_sampled_noise_chain, T (D + Jn) N multiplications and T W for nu, and
 * T (2 N + 2) for its sums; the strategy adds one pass over the node rows per game, (D + Jn) T (N - 1) for a best response.
 *
 * Returns the union of thrl_sampled_deviation's and thrl_sampled_noise_chain's lists: as thrl_sampled_deviation (with
 * THRL_SDN_POLICY for THRL_SD_POLICY), and THRL_ERR_BAD_CONFIG for n_nodes < 2, band_w < 1 or a scalar noise_prob outside
 * [0, 1] or NaN; THRL_ERR_UNSUPPORTED for n_nodes > THRL_STAT_MAX_CELLS or the working set; THRL_ERR_NULL for a missing
 * nprob[i] of a neural agent, npolicy, band_lo, band, noise_price or noise_reward.  All of these are decided before any
 * launch, the host-visible arguments and the working set before any pointer is looked at.
 */
#define THRL_SDN_POLICY 1
#define THRL_SDN_MAX_LDS (160 * 1024)
typedef struct {
    int32_t n_games;                 /* G >= 1: games of prob, nprob, dpolicy and npolicy */
    int32_t n_tuples;                /* T = prod_i n_actions_i <= THRL_TP_MAX_TUPLES     */
    int32_t n_prices;                /* D in [1, T]: the distinct prices                 */
    int32_t n_nodes;                 /* Jn in [2, THRL_STAT_MAX_CELLS]                   */
    int32_t band_w;                  /* W >= 1                                           */
    int32_t deviator;                /* delta in [0, N)                                  */
    int32_t dev_len;                 /* L >= 1                                           */
    int32_t n_steps;                 /* K in [L, THRL_DEV_MAX_STEPS]                     */
    int32_t dev_action;              /* fixed action index of delta, or -1               */
    int32_t row_begin;               /* rows stored: tau in [row_begin, row_begin + row_count) */
    int32_t row_count;
    int32_t flags;                   /* THRL_SDN_POLICY                                  */
    int32_t reserved[2];             /* 0                                                */
    int32_t kind[THRL_MAXA];         /* 0 = QTable, 1 = Reinforce, 2 = ActorCritic (3 = CAC is refused) */
    double  eps[THRL_MAXA];          /* QTable agents' epsilon in [0, 1], read when eps_g is NULL */
    double  gamma;                   /* in [0, 1], read when sweep_gamma is NULL         */
    double  ret_tol;                 /* >= 0                                             */
    double  noise_prob;              /* in [0, 1], read when noise_prob_g is NULL        */
    const double* eps_g;             /* device [N][G] or NULL                            */
    const double* sweep_gamma;       /* device [N][G] or NULL                            */
    const double* noise_prob_g;      /* device [G] or NULL                               */
    const float* prob[THRL_MAXA];    /* device [G][D][A_i] for the neural agents         */
    const float* nprob[THRL_MAXA];   /* device [G][Jn][A_i] for the neural agents        */
    const uint16_t* dpolicy;         /* device [G][N][D]                                 */
    const uint16_t* npolicy;         /* device [G][N][Jn]                                */
    const uint16_t* dev_policy;      /* device [G][D + Jn], with THRL_SDN_POLICY         */
    const int32_t* grp_first;        /* device [D + 1]                                   */
    const int32_t* grp_perm;         /* device [T]                                       */
    const double* reward;            /* device [N][T]                                    */
    const double* scaled;            /* device [N][T]                                    */
    const double* price;             /* device [T]                                       */
    const int32_t* band_lo;          /* device [T]                                       */
    const double* band;              /* device [T][W]                                    */
    const double* noise_price;       /* device [T]                                       */
    const double* noise_reward;      /* device [N][T]                                    */
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
} thrl_sampled_deviation_noise_args;
int thrl_sampled_deviation_noise(const thrl_cfg* cfg, const thrl_sampled_deviation_noise_args* args, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* THRL_SAMPLED_DEVIATION_NOISE_H */
