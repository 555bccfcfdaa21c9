// thrl_api_analysis.hip -- the extern "C" surface of libthrl_hip.so (see include/thrl.h), second half: the entry points
// of the post-training analyses.  Host logic only: an entry point makes its own checks in its own order, fills its
// module's Args, has the module's header lay out LDS and plans its grid with the helpers below.  thrl_host.h declares
// what it shares with thrl_api.hip (the error string, validate, fill_agents, reach_window).
#include <math.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "thrl_attractors.h"
#include "thrl_stationary.h"
#include "thrl_converge.h"
#include "thrl_crossplay.h"
#include "thrl_deviation.h"
#include "thrl_deviation_noise.h"
#include "thrl_equilibrium.h"
#include "thrl_equilibrium_noise.h"
#include "thrl_host.h"
#include "thrl_tuple_analysis.h"
#include "thrl_tuple_attractors.h"
#include "thrl_tuple_deviation_noise.h"
#include "thrl_tuple_equilibrium_noise.h"
#include "thrl_tuple_play.h"
#include "thrl_sampled.h"
#include "thrl_sampled_deviation.h"
#include "thrl_sampled_deviation_noise.h"
#include "thrl_sampled_noise.h"
#include "thrl_sampled_response.h"
#include "thrl_sampled_response_noise.h"
#include "thrl_tuple_stationary.h"

#include "../../include/thrl_response.h"
#include "../../include/thrl_response_noise.h"
#include "../../include/thrl_sampled_deviation.h"
#include "../../include/thrl_sampled_deviation_noise.h"

using namespace thrl;
using namespace thrl::host;

namespace thrl { int launch_group_stats(const thrl_group_stats_args* g, hipStream_t s); }   // thrl_stats.hip

namespace {

// power of two (a double with mantissa exactly 0.5 after frexp), positive and finite
bool pow2(double x) {
    int ex;
    return x > 0.0 && isfinite(x) && frexp(x, &ex) == 0.5;
}

// ---- argument checks that several entry points make, each at its own place in the order of its checks: THRL_OK, or
// the refusal with its message
int check_games_of(int n_games, const thrl_cfg* c) {            // the first n_games games of the config's tables
    const bool ok = n_games >= 1 && n_games <= c->n_games;
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", n_games, c->n_games);
}
int check_games(int n_games) {                                  // tuple form: the arrays are the caller's, any count
    return n_games >= 1 ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", n_games);
}
int check_horizon(int horizon) {
    const bool ok = horizon >= 1 && horizon <= THRL_DEV_MAX_HORIZON;
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "horizon=%d out of [1,%d]", horizon, THRL_DEV_MAX_HORIZON);
}
int check_rows(int row_begin, int row_count, int n_steps) {     // the slice of per-step rows a call writes
    if (row_begin < 0 || row_count < 0 || (int64_t)row_begin + row_count > n_steps)
        return fail(THRL_ERR_BAD_CONFIG, "rows [%d, %d + %d) outside [0, n_steps=%d)", row_begin, row_begin, row_count,
                    n_steps);
    return THRL_OK;
}
int check_steps_rows(int n_steps, int row_begin, int row_count) {       // the walks: no step at all is allowed
    if (n_steps < 0 || n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [0,%d]", n_steps, THRL_DEV_MAX_STEPS);
    return check_rows(row_begin, row_count, n_steps);
}
// the deviator, the deviation's length and the steps; then the action: the parts of check_deviation that a call without a
// horizon makes too (thrl_deviation_noise)
int check_deviator(const thrl_cfg* c, int deviator, int dev_len, int n_steps) {
    const int N = c->n_agents;
    if (deviator < 0 || deviator >= N) return fail(THRL_ERR_BAD_CONFIG, "deviator=%d out of [0,%d)", deviator, N);
    if (dev_len < 1) return fail(THRL_ERR_BAD_CONFIG, "dev_len=%d must be >= 1", dev_len);
    if (n_steps < dev_len || n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [dev_len=%d, %d]", n_steps, dev_len, THRL_DEV_MAX_STEPS);
    return THRL_OK;
}
int check_dev_action(const thrl_cfg* c, int deviator, int dev_action) {
    if (dev_action < -1 || dev_action >= c->n_actions[deviator])
        return fail(THRL_ERR_BAD_CONFIG, "dev_action=%d: -1 (best response) or an action of agent %d in [0,%d)", dev_action,
                    deviator, c->n_actions[deviator]);
    return THRL_OK;
}
int check_deviation(const thrl_cfg* c, int deviator, int dev_len, int n_steps, int horizon, int dev_action) {
    if (const int rc = check_deviator(c, deviator, dev_len, n_steps)) return rc;
    if (const int rc = check_horizon(horizon)) return rc;
    return check_dev_action(c, deviator, dev_action);
}
int check_tol(double tol, const char* tol_name) {               // a tolerance: >= 0, which refuses NaN
    return tol >= 0.0 ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "%s=%g must be >= 0", tol_name, tol);
}
int check_iters_tol(int max_iters, double tol, const char* iters_name = "max_iters", const char* tol_name = "tol") {
    if (max_iters < 1 || max_iters > THRL_STAT_MAX_ITERS)
        return fail(THRL_ERR_BAD_CONFIG, "%s=%d out of [1,%d]", iters_name, max_iters, THRL_STAT_MAX_ITERS);
    return check_tol(tol, tol_name);
}
// ---- the checks of the calls on the cells of noisy play (thrl_stationary, thrl_equilibrium_noise,
// thrl_deviation_noise), `call` their name
int check_tuple_limit(const thrl_cfg* c, const char* call, int* T) {   // T = prod n_actions needs no plan
    int64_t T64 = 1;
    for (int i = 0; i < c->n_agents; i++) {
        T64 *= c->n_actions[i];
        if (T64 > THRL_EQ_MAX_TUPLES)
            return fail(THRL_ERR_UNSUPPORTED, "%s: more than %d action tuples (prod n_actions)", call, THRL_EQ_MAX_TUPLES);
    }
    *T = (int)T64;
    return THRL_OK;
}
int check_cells_band(int n_cells, int band_w) {
    const bool ok = n_cells >= 1 && band_w >= 1;
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "n_cells=%d and band_w=%d must be >= 1", n_cells, band_w);
}
int check_noise_prob(const double* noise_prob_g, double noise_prob) {  // the host-visible value; the array is the device's
    const bool ok = noise_prob_g || (noise_prob > 0.0 && noise_prob <= 1.0);
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "noise_prob=%g out of (0, 1]", noise_prob);
}
int check_cell_limit(const char* call, int n_cells) {
    const bool ok = n_cells <= THRL_STAT_MAX_CELLS;
    return ok ? THRL_OK : fail(THRL_ERR_UNSUPPORTED, "%s: n_cells=%d, at most %d", call, n_cells, THRL_STAT_MAX_CELLS);
}
// ---- the checks of the calls on sampled play (thrl_sampled_chain, thrl_sampled_noise_chain, thrl_sampled_response,
// thrl_sampled_response_noise, thrl_sampled_deviation, thrl_sampled_deviation_noise)
int check_prices(int n_prices, int n_tuples) {
    const bool ok = n_prices >= 1 && n_prices <= n_tuples;
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "n_prices=%d out of [1, n_tuples=%d]", n_prices, n_tuples);
}
int check_nodes_band(int n_nodes, int band_w) {
    const bool ok = n_nodes >= 2 && band_w >= 1;
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "n_nodes=%d must be >= 2 and band_w=%d >= 1", n_nodes, band_w);
}
int check_noise_prob_closed(const double* noise_prob_g, double noise_prob) {    // p = 0 allowed: the chains under noise
    const bool ok = noise_prob_g || (noise_prob >= 0.0 && noise_prob <= 1.0);
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "noise_prob=%g out of [0, 1]", noise_prob);
}
int check_node_limit(const char* call, int n_nodes) {
    const bool ok = n_nodes <= THRL_STAT_MAX_CELLS;
    return ok ? THRL_OK : fail(THRL_ERR_UNSUPPORTED, "%s: n_nodes=%d, at most %d", call, n_nodes, THRL_STAT_MAX_CELLS);
}
int lds_refusal(const char* call, int64_t need, int N, int n_cells) {
    return fail(THRL_ERR_UNSUPPORTED, "%s: %lld bytes of LDS per game (N=%d, n_cells=%d)", call, (long long)need, N, n_cells);
}
int missing(const char* names) { return fail(THRL_ERR_NULL, "%s is NULL", names); }
int missing_rows(int i) { return fail(THRL_ERR_NULL, "prob[%d] / nprob[%d] is NULL", i, i); }    // a network's, prices and nodes
int missing_q(const char* flag) { return fail(THRL_ERR_NULL, "q is NULL without %s", flag); }
int check_eps(int N, const int32_t* kind, const double* eps) {  // the scalar epsilons of the QTable agents (no eps_g)
    for (int i = 0; i < N; i++)
        if (kind[i] == 0 && !(eps[i] >= 0.0 && eps[i] <= 1.0))
            return fail(THRL_ERR_BAD_CONFIG, "eps[%d]=%g out of [0, 1]", i, eps[i]);
    return THRL_OK;
}
int check_agents_mask(int agents, int N) {
    const bool ok = agents != 0 && !(agents & ~((1 << N) - 1));
    return ok ? THRL_OK : fail(THRL_ERR_BAD_CONFIG, "agents=0x%x: a non-empty mask of agents in [0,%d)", agents, N);
}
int check_gamma(const double* gamma, int N, int agents) {       // the host's gammas of the solved agents (no sweep_gamma)
    for (int i = 0; i < N; i++)
        if (((agents >> i) & 1) && !(gamma[i] >= 0.0 && gamma[i] < 1.0))
            return fail(THRL_ERR_BAD_CONFIG, "agent %d: gamma=%g: the equilibrium check needs gamma in [0, 1)", i, gamma[i]);
    return THRL_OK;
}
int check_gamma(const thrl_cfg* c, int agents) { return check_gamma(c->gamma, c->n_agents, agents); }   // the config's

// ---- planning that several entry points share
// tstride[i] = prod_{j > i} n_actions[j] (agent 0 slowest); n_actions may be NULL where the Args carry AgentParams
void tuple_strides(const thrl_cfg* c, int32_t* n_actions, int32_t* tstride) {
    int ts = 1;
    for (int i = c->n_agents - 1; i >= 0; i--) {
        if (n_actions) n_actions[i] = c->n_actions[i];
        tstride[i] = ts; ts *= c->n_actions[i];
    }
}

// A game's P policy entries, one per table row, agent i's from row_off[i] (row_off[N] = P is the caller's, where its
// array has that slot); table_off and n_actions may be NULL.  Returns P.
int table_rows(const AgentParams* ag, int N, int32_t* row_off, int32_t* table_off, int32_t* n_actions) {
    int P = 0;
    for (int i = 0; i < N; i++) {
        row_off[i] = P;
        if (table_off) table_off[i] = ag[i].table_off;
        if (n_actions) n_actions[i] = ag[i].n_actions;
        P += ag[i].rows;
    }
    return P;
}

// The staged window of a kernel that streams a game's tables: the game's block widened to 16-byte chunks at both ends.
// Its bytes and *staged = 1, or 0 and 0 when it is over the budget or q is not 16-byte aligned.
int32_t staged_window(const thrl_cfg* c, const void* q, int budget, int32_t* staged) {
    const int64_t esz = c->q_dtype == 1 ? 8 : 4, vec = 16 / esz;
    const int64_t lds = (((int64_t)thrl_table_stride(c) + 2 * vec) * esz + 15) & ~(int64_t)15;
    *staged = lds <= budget && ((uintptr_t)q & 15) == 0;
    return *staged ? (int32_t)lds : 0;
}

// The policy windows and the scale LUT of the walks from a state (thrl_deviation, thrl_crossplay): agent i's reachable
// rows [win_lo, win_lo + win_n) and x_0's row from entry pol_off[i] (pol_off[N] = *entries), its scaled actions from
// LUT entry lut_off[i] (*lut_n in all)
void reach_tables(const thrl_cfg* c, int32_t* win_lo, int32_t* win_n, int32_t* pol_off, int32_t* lut_off, int32_t* entries,
                  int32_t* lut_n) {
    int lo[THRL_MAXA], hi[THRL_MAXA];
    reach_window(c, lo, hi);
    *entries = *lut_n = 0;
    for (int i = 0; i < c->n_agents; i++) {
        win_lo[i] = lo[i];
        win_n[i] = hi[i] - lo[i] + 1;
        pol_off[i] = *entries;
        *entries += win_n[i] + 1;                    // + x_0's row
        lut_off[i] = *lut_n;
        *lut_n += c->n_actions[i];
    }
    pol_off[c->n_agents] = *entries;
}

// CUs and LDS per CU of the current device, for the grids of the analyses.  Not dev_info() of thrl_api.hip: that one
// caches and assumes an MI355X when no device is visible (the training plans' host tests); an analysis about to launch
// must fail without one.
int cu_figures(int* cus, int* lds_cu) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    return THRL_OK;
}

// A grid of blocks that loop over G games: per CU as many as LDS allows (lds_bytes == 0: no LDS, no limit from it), at
// most max_per_cu and at least one; never more blocks than games
int grid_for(int cus, int lds_cu, int lds_bytes, int max_per_cu, int G) {
    int per_cu = max_per_cu;
    if (lds_bytes > 0 && lds_cu > 0 && lds_cu / lds_bytes < per_cu) per_cu = lds_cu / lds_bytes > 0 ? lds_cu / lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    return (int)(want < G ? want : G);
}

}  // namespace

extern "C" {

int thrl_group_stats(const thrl_group_stats_args* g, void* stream) {
    if (!g) return fail(THRL_ERR_NULL, "args is NULL");
    if (const int rc = check_games(g->n_games)) return rc;
    if (g->n_agents < 1 || g->n_agents > THRL_MAXA)
        return fail(THRL_ERR_BAD_CONFIG, "n_agents=%d out of [1,%d]", g->n_agents, THRL_MAXA);
    if (g->n_episodes < 0) return fail(THRL_ERR_BAD_CONFIG, "n_episodes=%d must be >= 0", g->n_episodes);
    if (g->n_groups < 1) return fail(THRL_ERR_BAD_CONFIG, "n_groups=%d must be >= 1", g->n_groups);
    if (g->n_bins < 1 || g->n_bins > THRL_STATS_MAX_BINS)
        return fail(THRL_ERR_UNSUPPORTED, "n_bins=%d out of [1,%d]", g->n_bins, THRL_STATS_MAX_BINS);
    if (g->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved must be 0");
    if (!g->game_reward_log || !g->game_action_log || !g->group_of || !g->perm || !g->seg_off || !g->hist || !g->sums
        || !g->minmax)
        return fail(THRL_ERR_NULL, "game_reward_log / game_action_log / group_of / perm / seg_off / hist / sums / minmax "
                                   "is NULL");
    // group ids, and the largest group of this call (the int64 bound of include/thrl.h)
    int64_t n_max = 0;
    {
        std::vector<int64_t> cnt((size_t)g->n_groups, 0);
        for (int i = 0; i < g->n_games; i++) {
            const int32_t k = g->group_of[i];
            if (k < 0 || k >= g->n_groups)
                return fail(THRL_ERR_BAD_CONFIG, "group_of[%d]=%d out of [0,%d)", i, k, g->n_groups);
            if (++cnt[(size_t)k] > n_max) n_max = cnt[(size_t)k];
        }
    }
    const int Q = 2 * g->n_agents + 1;
    for (int q = 0; q < Q; q++) {
        const double lo = g->lo[q], hi = g->hi[q];
        if (!isfinite(lo) || !isfinite(hi) || !(hi > lo))
            return fail(THRL_ERR_BAD_CONFIG, "quantity %d: range [%g, %g) needs finite lo < hi", q, lo, hi);
        if (!(g->inv_w[q] > 0.0) || !isfinite(g->inv_w[q]))
            return fail(THRL_ERR_BAD_CONFIG, "quantity %d: inv_w=%g must be B / (hi - lo)", q, g->inv_w[q]);
        // the int64 bound of include/thrl.h for this call's games
        const double M = 16.0 * fmax(fabs(lo), fabs(hi));
        const double n = (double)n_max;
        for (int k = 0; k < 2; k++) {
            const double sc = g->scale[q][k];
            const double need = (k == 0 ? M : M * M) * n * sc;
            if (!pow2(sc) || !(need <= 4611686018427387904.0))
                return fail(THRL_ERR_BAD_CONFIG, "quantity %d: scale[%d]=%g must be a power of two with "
                            "scale * M%s * n <= 2^62 (M = %g, n = %lld: the largest group)", q, k, sc, k ? "^2" : "", M,
                            (long long)n_max);
        }
    }
    if (g->n_episodes == 0) return THRL_OK;
    const int e = thrl::launch_group_stats(g, (hipStream_t)stream);
    return e ? hip_fail(e, "k_group_stats launch") : THRL_OK;
}

int thrl_deviation(const thrl_cfg* c, const void* q, const thrl_deviation_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if ((rc = check_deviation(c, x->deviator, x->dev_len, x->n_steps, x->horizon, x->dev_action)) != THRL_OK) return rc;
    if ((rc = check_rows(x->row_begin, x->row_count, x->n_steps)) != THRL_OK) return rc;
    if (!q || !x->state0 || !x->mu || !x->lam || !x->mu_post || !x->lam_post || !x->ret_step || !x->act_dev
        || !x->cycle_reward || !x->cycle_action || !x->gain)
        return fail(THRL_ERR_NULL, "q / state0 / mu / lam / mu_post / lam_post / ret_step / act_dev / cycle_reward / "
                                   "cycle_action / gain is NULL");
    DevArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.d = x->deviator; a.L = x->dev_len; a.K = x->n_steps; a.H = x->horizon;
    a.dev_action = x->dev_action; a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a.ag, &a.env);
    reach_tables(c, a.win_lo, a.win_n, a.pol_off, a.lut_off, &a.pol_entries, &a.lut_n);
    const int entries = a.pol_entries, lut_n = a.lut_n;
    int max_a = 0;
    for (int i = 0; i < N; i++)
        if (c->n_actions[i] > max_a) max_a = c->n_actions[i];
    a.pol_bytes = max_a <= 256 ? 1 : 2;
    const int64_t lds = (int64_t)((lut_n * 8 + 15) & ~15) + (int64_t)kDevTile * entries * a.pol_bytes;
    a.staged = lut_n <= kDevMaxLut && lds <= kDevLdsBudget;
    a.lds_bytes = a.staged ? (int32_t)lds : 0;
    a.q = q; a.state0 = x->state0; a.sweep_gamma = x->sweep_gamma;
    a.mu = x->mu; a.lam = x->lam; a.mu_post = x->mu_post; a.lam_post = x->lam_post; a.ret_step = x->ret_step;
    a.act_dev = x->act_dev; a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action; a.gain = x->gain;
    a.reward_rows = x->reward_rows; a.action_rows = x->action_rows;
    const int e = thrl::launch_deviation(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_deviation launch") : THRL_OK;
}

int thrl_policy_track(const thrl_cfg* c, const void* q, const thrl_policy_track_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->window < 1) return fail(THRL_ERR_BAD_CONFIG, "window=%lld must be >= 1", (long long)x->window);
    if (x->flags & ~THRL_TRACK_BASELINE) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    // validate() caps every agent at 32,000 actions, so each greedy action fits a 16-bit policy entry (thrl.h's
    // "more than 65,536 actions" is refused there, with THRL_ERR_BAD_CONFIG)
    if (x->q_conv && (!x->state || !x->state_conv))
        return fail(THRL_ERR_BAD_CONFIG, "q_conv needs state and state_conv");
    if (!q || !x->policy || !x->stable_since || !x->converged_at || !x->conv_since || !x->changes)
        return fail(THRL_ERR_NULL, "q / policy / stable_since / converged_at / conv_since / changes is NULL");
    TrackArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.baseline = (x->flags & THRL_TRACK_BASELINE) ? 1 : 0;
    a.stride = (int64_t)thrl_table_stride(c);
    a.episode = x->episode; a.window = x->window;
    AgentParams ag[THRL_MAXA];
    fill_agents(c, ag, nullptr);
    a.P = a.row_off[N] = table_rows(ag, N, a.row_off, a.table_off, a.n_actions);
    a.lds_bytes = staged_window(c, q, kTrackLdsBudget, &a.staged);
    a.q = q; a.policy = x->policy; a.stable_since = x->stable_since; a.converged_at = x->converged_at;
    a.conv_since = x->conv_since; a.changes = x->changes; a.n_converged = x->n_converged;
    a.state = x->state; a.q_conv = x->q_conv; a.state_conv = x->state_conv;
    // enough one-wave blocks to fill every CU as far as LDS allows, each looping over games
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTrackMaxBlocksPerCu, a.G);
    const int e = thrl::launch_policy_track(a, c->q_dtype, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_policy_track launch") : THRL_OK;
}

// The greedy policy of the first G games of q into policy [G][P], 2 bytes per table row (k_xplay_extract): the pass
// thrl_crossplay and thrl_attractors run without their POLICY_GIVEN flag.
static int extract_policies(const thrl_cfg* c, const void* q, int G, uint16_t* policy, void* stream) {
    const int N = c->n_agents;
    int rc;
    AgentParams ag[THRL_MAXA];
    fill_agents(c, ag, nullptr);
    XpExtractArgs e;
    memset(&e, 0, sizeof(e));
    e.G = G; e.N = N;
    e.P = e.row_off[N] = table_rows(ag, N, e.row_off, e.table_off, e.n_actions);
    e.stride = (int64_t)thrl_table_stride(c);
    e.lds_bytes = staged_window(c, q, kXpExtractLdsBudget, &e.staged);
    e.q = q; e.policy = policy;
    // enough one-wave blocks to fill every CU as far as LDS allows, each looping over games
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, e.lds_bytes, kXpExtractMaxBlocksPerCu, e.G);
    const int err = thrl::launch_xplay_extract(e, c->q_dtype, grid, (hipStream_t)stream);
    return err ? hip_fail(err, "k_xplay_extract launch") : THRL_OK;
}

int thrl_crossplay(const thrl_cfg* c, const void* q, const thrl_crossplay_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if (x->n_matches < 1) return fail(THRL_ERR_BAD_CONFIG, "n_matches=%d must be >= 1", x->n_matches);
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if ((rc = check_horizon(x->horizon)) != THRL_OK) return rc;
    if ((rc = check_steps_rows(x->n_steps, x->row_begin, x->row_count)) != THRL_OK) return rc;
    if (x->flags & ~THRL_XPLAY_POLICY_GIVEN) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    // validate() caps every agent at 32,000 actions, so each greedy action fits a 16-bit policy entry (thrl.h's
    // "more than 65,536 actions" is refused there, with THRL_ERR_BAD_CONFIG)
    const bool given = (x->flags & THRL_XPLAY_POLICY_GIVEN) != 0;
    if (!x->seat || !x->state0 || !x->policy || !x->mu || !x->lam || !x->cycle_reward || !x->cycle_action)
        return fail(THRL_ERR_NULL, "seat / state0 / policy / mu / lam / cycle_reward / cycle_action is NULL");
    if (!given && !q) return fail(THRL_ERR_NULL, "q is NULL without THRL_XPLAY_POLICY_GIVEN");
    AgentParams ag[THRL_MAXA];
    EnvParams env;
    fill_agents(c, ag, &env);
    // one streaming pass over q: policy[g] for every g < G
    if (!given && (rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;

    XpWalkArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.M = x->n_matches; a.N = N; a.H = x->horizon; a.K = x->n_steps;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.env = env;
    for (int i = 0; i < N; i++) a.ag[i] = ag[i];
    a.P = table_rows(ag, N, a.row_off, nullptr, nullptr);
    reach_tables(c, a.win_lo, a.win_n, a.pol_off, a.lut_off, &a.pol_entries, &a.lut_n);
    const int entries = a.pol_entries, lut_n = a.lut_n;
    a.use_lut = lut_n <= kDevMaxLut;
    const int64_t lut_bytes = a.use_lut ? (int64_t)((lut_n * 8 + 15) & ~15) : 0;
    const int64_t lds = lut_bytes + (int64_t)kXpTile * entries * 2;
    a.staged = lds <= kXpLdsBudget;
    a.lds_bytes = (int32_t)(a.staged ? lds : lut_bytes);
    a.policy = x->policy; a.seat = x->seat; a.state0 = x->state0;
    a.mu = x->mu; a.lam = x->lam; a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action;
    a.reward_rows = x->reward_rows; a.action_rows = x->action_rows;
    const int e = thrl::launch_xplay_walk(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_xplay_walk launch") : THRL_OK;
}

// n_tuples must be the game's own: prod_i n_actions_i, at most THRL_TP_MAX_TUPLES
static int tuple_count_check(const thrl_cfg* c, int n_tuples) {
    if (n_tuples < 1) return fail(THRL_ERR_BAD_CONFIG, "n_tuples=%d must be >= 1", n_tuples);
    if (n_tuples > THRL_TP_MAX_TUPLES)
        return fail(THRL_ERR_UNSUPPORTED, "n_tuples=%d, at most %d", n_tuples, THRL_TP_MAX_TUPLES);
    int64_t prod = 1;
    for (int i = 0; i < c->n_agents; i++) {
        prod *= c->n_actions[i];
        if (prod > THRL_TP_MAX_TUPLES) break;
    }
    if (prod != n_tuples)
        return fail(THRL_ERR_BAD_CONFIG, "n_tuples=%d is not the product of the agents' action counts", n_tuples);
    return THRL_OK;
}

// kinds of a game in tuple form: CAC has no tuples, a network has 2..32 actions
static int tuple_kinds_check(const thrl_cfg* c, const int32_t* kind) {
    for (int i = 0; i < c->n_agents; i++) {
        if (kind[i] == 3)
            return fail(THRL_ERR_UNSUPPORTED, "agent %d is a CAC agent: its action is continuous, the game has no tuples", i);
        if (kind[i] < 0 || kind[i] > 3) return fail(THRL_ERR_BAD_CONFIG, "agent %d: kind=%d", i, kind[i]);
        if (kind[i] != 0 && (c->n_actions[i] < 2 || c->n_actions[i] > 32))
            return fail(THRL_ERR_BAD_CONFIG, "neural agent %d: actions=%d out of [2,32]", i, c->n_actions[i]);
    }
    return THRL_OK;
}

// the extraction of thrl_tuple_policy and thrl_price_policy: n_prices states per game, shared (price_stride = 0) or
// per game, into out [G][N][n_prices]
static int extract_at_prices(const thrl_cfg* c, const void* q, const int32_t* kind, const float* const* nn_params, int G,
                             int n_prices, const double* price, int64_t price_stride, uint16_t* out, void* stream) {
    const int N = c->n_agents;
    TpPolicyArgs a;
    memset(&a, 0, sizeof(a));
    fill_agents(c, a.ag, nullptr);
    a.G = G; a.N = N; a.T = n_prices;
    a.stride = (int64_t)thrl_table_stride(c);
    for (int i = 0; i < N; i++) {
        if (kind[i] == 0) {
            a.q_agent[a.n_q++] = i;
        } else {
            if (!nn_params[i]) return fail(THRL_ERR_NULL, "nn_params[%d] is NULL", i);
            const int j = a.n_nn++;
            a.nn_agent[j] = i;
            a.nn_actions[j] = c->n_actions[i];
            a.nn_stride[j] = kind[i] == 2 ? (int32_t)thrl_ac_param_count(c->n_actions[i])
                                          : (int32_t)thrl_nn_param_count(c->n_actions[i]);
            a.nn_params[j] = nn_params[i];
        }
    }
    if (a.n_q > 0 && !q) return fail(THRL_ERR_NULL, "q is NULL with a QTable agent in the game");
    a.q = q; a.price = price; a.price_stride = price_stride; a.policy = out;
    const int e = thrl::launch_tp_policy(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_tp_qtable / k_tp_neural launch") : THRL_OK;
}

int thrl_tuple_policy(const thrl_cfg* c, const void* q, const thrl_tuple_policy_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->price || !x->tuple_policy) return fail(THRL_ERR_NULL, "price / tuple_policy is NULL");
    return extract_at_prices(c, q, x->kind, x->nn_params, x->n_games, x->n_tuples, x->price, 0, x->tuple_policy, stream);
}

int thrl_price_policy(const thrl_cfg* c, const void* q, const thrl_price_policy_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->flags & ~THRL_PP_PER_GAME) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if (x->n_prices < 1) return fail(THRL_ERR_BAD_CONFIG, "n_prices=%d must be >= 1", x->n_prices);
    if (x->n_prices > THRL_STAT_MAX_CELLS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_price_policy: n_prices=%d, at most %d", x->n_prices, THRL_STAT_MAX_CELLS);
    if (!x->price || !x->price_policy) return fail(THRL_ERR_NULL, "price / price_policy is NULL");
    return extract_at_prices(c, q, x->kind, x->nn_params, x->n_games, x->n_prices, x->price,
                             (x->flags & THRL_PP_PER_GAME) ? x->n_prices : 0, x->price_policy, stream);
}

int thrl_tuple_walk(const thrl_cfg* c, const thrl_tuple_walk_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if (x->n_matches < 1) return fail(THRL_ERR_BAD_CONFIG, "n_matches=%d must be >= 1", x->n_matches);
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if ((rc = check_horizon(x->horizon)) != THRL_OK) return rc;
    if ((rc = check_steps_rows(x->n_steps, x->row_begin, x->row_count)) != THRL_OK) return rc;
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->seat || !x->start || !x->tuple_policy || !x->reward || !x->scaled || !x->mu || !x->lam || !x->cycle_reward
        || !x->cycle_action)
        return fail(THRL_ERR_NULL, "seat / start / tuple_policy / reward / scaled / mu / lam / cycle_reward / cycle_action is NULL");
    TpWalkArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.M = x->n_matches; a.N = N; a.T = x->n_tuples; a.H = x->horizon; a.K = x->n_steps;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    tuple_strides(c, a.n_actions, a.tstride);
    const int64_t lds = (int64_t)2 * N * a.T * 8;
    a.in_lds = lds <= kTpLdsBudget;
    a.lds_bytes = a.in_lds ? (int32_t)lds : 0;
    a.policy = x->tuple_policy; a.seat = x->seat; a.start = x->start; a.reward = x->reward; a.scaled = x->scaled;
    a.mu = x->mu; a.lam = x->lam; a.cycle_start = x->cycle_start;
    a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action;
    a.reward_rows = x->reward_rows; a.action_rows = x->action_rows;
    const int e = thrl::launch_tp_walk(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_tp_walk launch") : THRL_OK;
}

int thrl_tuple_deviation(const thrl_cfg* c, const thrl_tuple_deviation_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if ((rc = check_deviation(c, x->deviator, x->dev_len, x->n_steps, x->horizon, x->dev_action)) != THRL_OK) return rc;
    if ((rc = check_rows(x->row_begin, x->row_count, x->n_steps)) != THRL_OK) return rc;
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->start || !x->tuple_policy || !x->reward || !x->scaled || !x->mu || !x->lam || !x->mu_post || !x->lam_post
        || !x->ret_step || !x->act_dev || !x->cycle_reward || !x->cycle_action || !x->gain)
        return fail(THRL_ERR_NULL, "start / tuple_policy / reward / scaled / mu / lam / mu_post / lam_post / ret_step / "
                                   "act_dev / cycle_reward / cycle_action / gain is NULL");
    TaDevArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.H = x->horizon; a.d = x->deviator; a.L = x->dev_len;
    a.K = x->n_steps; a.dev_action = x->dev_action; a.row_begin = x->row_begin; a.row_count = x->row_count;
    tuple_strides(c, a.n_actions, a.tstride);
    a.gamma_d = c->gamma[x->deviator];
    const int64_t lds = (int64_t)2 * N * a.T * 8;
    a.in_lds = lds <= kTaDevLdsBudget;
    a.lds_bytes = a.in_lds ? (int32_t)lds : 0;
    a.start = x->start; a.policy = x->tuple_policy; a.reward = x->reward; a.scaled = x->scaled;
    a.sweep_gamma = x->sweep_gamma;
    a.mu = x->mu; a.lam = x->lam; a.mu_post = x->mu_post; a.lam_post = x->lam_post; a.ret_step = x->ret_step;
    a.act_dev = x->act_dev; a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action; a.gain = x->gain;
    a.reward_rows = x->reward_rows; a.action_rows = x->action_rows;
    const int e = thrl::launch_ta_deviation(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ta_deviation launch") : THRL_OK;
}

int thrl_tuple_equilibrium(const thrl_cfg* c, const thrl_tuple_equilibrium_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if ((rc = check_agents_mask(x->agents, N)) != THRL_OK) return rc;
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->sweep_gamma && (rc = check_gamma(c, x->agents)) != THRL_OK) return rc;
    if (!x->start || !x->tuple_policy || !x->reward || !x->mu || !x->lam || !x->iters || !x->n_diff_all
        || !x->n_diff_on || !x->loss_all || !x->loss_on || !x->loss_all_mean || !x->loss_on_mean || !x->v_on)
        return fail(THRL_ERR_NULL, "start / tuple_policy / reward / mu / lam / iters / n_diff_all / n_diff_on / loss_all / "
                                   "loss_on / loss_all_mean / loss_on_mean / v_on is NULL");
    TaEqArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.agents = x->agents;
    tuple_strides(c, a.n_actions, a.tstride);
    for (int i = 0; i < N; i++) a.gamma[i] = c->gamma[i];
    thrl::ta_eq_layout(a);
    a.start = x->start; a.policy = x->tuple_policy; a.reward = x->reward; a.sweep_gamma = x->sweep_gamma;
    a.mu = x->mu; a.lam = x->lam; a.iters = x->iters; a.n_diff_all = x->n_diff_all; a.n_diff_on = x->n_diff_on;
    a.loss_all = x->loss_all; a.loss_on = x->loss_on; a.loss_all_mean = x->loss_all_mean;
    a.loss_on_mean = x->loss_on_mean; a.v_on = x->v_on;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within THRL_TP_MAX_TUPLES
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_equilibrium: %d bytes of LDS per game, the device has %d", a.lds_bytes, lds_cu);
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTaEqMaxBlocksPerCu, a.G);
    const int e = thrl::launch_ta_equilibrium(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ta_equilibrium launch") : THRL_OK;
}

int thrl_tuple_attractors(const thrl_cfg* c, const thrl_tuple_attractors_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->reserved != 0 || x->reserved2 != 0)
        return fail(THRL_ERR_BAD_CONFIG, "reserved=%d, %d must be 0", x->reserved, x->reserved2);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->start || !x->tuple_policy || !x->reward || !x->scaled || !x->n_attr || !x->mu_max || !x->n_cycle_states
        || !x->rep || !x->lam || !x->basin || !x->cycle_reward || !x->cycle_action || !x->rep_x0 || !x->mu_x0 || !x->slot_x0)
        return fail(THRL_ERR_NULL, "start / tuple_policy / reward / scaled / n_attr / mu_max / n_cycle_states / rep / lam / "
                                   "basin / cycle_reward / cycle_action / rep_x0 / mu_x0 / slot_x0 is NULL");
    if (x->start_w && (!x->start_mass || !x->start_mass_other || !x->start_reward))
        return fail(THRL_ERR_NULL, "start_mass / start_mass_other / start_reward is NULL with start_w given");
    TatArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples;
    while ((1 << a.L) < a.T) a.L++;
    tuple_strides(c, a.n_actions, a.tstride);
    thrl::tat_layout(a);
    a.start = x->start; a.policy = x->tuple_policy; a.reward = x->reward; a.scaled = x->scaled; a.start_w = x->start_w;
    a.n_attr = x->n_attr; a.mu_max = x->mu_max; a.n_cycle_states = x->n_cycle_states;
    a.rep = x->rep; a.lam = x->lam; a.basin = x->basin; a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action;
    a.rep_x0 = x->rep_x0; a.mu_x0 = x->mu_x0; a.slot_x0 = x->slot_x0;
    a.start_mass = x->start_mass; a.start_mass_other = x->start_mass_other; a.start_reward = x->start_reward;
    a.tuple_rep = x->tuple_rep; a.tuple_mu = x->tuple_mu;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within THRL_TP_MAX_TUPLES
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_attractors: %d bytes of LDS per game, the device has %d", a.lds_bytes, lds_cu);
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTatMaxBlocksPerCu, a.G);
    const int e = thrl::launch_tuple_attractors(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ta_attractors launch") : THRL_OK;
}

int thrl_tuple_stationary(const thrl_cfg* c, const thrl_tuple_stationary_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked before the device is touched
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags & ~THRL_TS_START_TUPLE) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (x->n_cells < 1 || x->band_w < 1)
        return fail(THRL_ERR_BAD_CONFIG, "n_cells=%d and band_w=%d must be >= 1", x->n_cells, x->band_w);
    if ((rc = check_iters_tol(x->max_iters, x->tol)) != THRL_OK) return rc;
    if (!x->noise_prob_g && !(x->noise_prob > 0.0 && x->noise_prob <= 1.0))
        return fail(THRL_ERR_BAD_CONFIG, "noise_prob=%g out of (0, 1]", x->noise_prob);
    if (x->n_cells > THRL_STAT_MAX_CELLS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_stationary: n_cells=%d, at most %d", x->n_cells, THRL_STAT_MAX_CELLS);
    const bool start_tuple = (x->flags & THRL_TS_START_TUPLE) != 0;
    if (!x->tuple_policy || !x->cell_policy || !x->cell_w || !x->reward || !x->scaled || !x->price || !x->band_lo || !x->band
        || !x->noise_reward || !x->noise_price)
        return fail(THRL_ERR_NULL, "tuple_policy / cell_policy / cell_w / reward / scaled / price / band_lo / band / "
                                   "noise_reward / noise_price is NULL");
    if (!x->iters || !x->change || !x->mass || !x->stat_reward || !x->stat_action || !x->stat_price)
        return fail(THRL_ERR_NULL, "iters / change / mass / stat_reward / stat_action / stat_price is NULL");
    if (start_tuple && !x->start) return fail(THRL_ERR_NULL, "start is NULL with THRL_TS_START_TUPLE");

    TsArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.J = x->n_cells; a.W = x->band_w;
    a.max_iters = x->max_iters; a.start_tuple = start_tuple;
    a.noise_prob = x->noise_prob; a.tol = x->tol;
    tuple_strides(c, a.n_actions, a.tstride);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0) a.neural_mask |= 1 << i;
    thrl::ts_layout(a);                              // the working set of include/thrl.h
    a.noise_prob_g = x->noise_prob_g; a.start = x->start; a.tuple_policy = x->tuple_policy; a.cell_policy = x->cell_policy;
    a.cell_w = x->cell_w; a.reward = x->reward; a.scaled = x->scaled; a.price = x->price; a.band_lo = x->band_lo;
    a.band = x->band; a.noise_reward = x->noise_reward; a.noise_price = x->noise_price;
    a.iters = x->iters; a.change = x->change; a.mass = x->mass; a.stat_reward = x->stat_reward;
    a.stat_action = x->stat_action; a.stat_price = x->stat_price; a.pi = x->pi;
    a.n_switch = x->n_switch; a.unresolved = x->unresolved;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within the limits on T and J
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_stationary: %d bytes of LDS per game (T=%d, n_cells=%d), the device has %d",
                    a.lds_bytes, a.T, a.J, lds_cu);
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTsMaxBlocksPerCu, a.G);
    const int e = thrl::launch_tuple_stationary(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ts_switch / k_ts_chain launch") : THRL_OK;
}

int thrl_tuple_equilibrium_noise(const thrl_cfg* c, const thrl_tuple_equilibrium_noise_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_tuple_stationary's checks in its order, with the agents and their gammas as thrl_equilibrium_noise checks them;
    // every host-visible argument is checked before the device is touched
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags != 0) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = check_agents_mask(x->agents, N)) != THRL_OK) return rc;
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->sweep_gamma && (rc = check_gamma(x->gamma, N, x->agents)) != THRL_OK) return rc;
    if ((rc = check_cells_band(x->n_cells, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_sweeps, x->eval_tol, "max_sweeps", "eval_tol")) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_cell_limit("thrl_tuple_equilibrium_noise", x->n_cells)) != THRL_OK) return rc;
    TenArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.J = x->n_cells; a.W = x->band_w;
    const int64_t need = thrl::ten_layout(a);            // the working set of include/thrl.h
    if (need > THRL_TEN_MAX_LDS) return lds_refusal("thrl_tuple_equilibrium_noise", need, N, x->n_cells);
    if (!x->tuple_policy || !x->cell_policy || !x->reward || !x->band_lo || !x->band || !x->noise_reward)
        return missing("tuple_policy / cell_policy / reward / band_lo / band / noise_reward");
    if (!x->iters || !x->sweeps || !x->n_diff_tuples || !x->n_diff_cells || !x->loss_all || !x->loss_tuples_mean
        || !x->loss_cells_mean)
        return missing("iters / sweeps / n_diff_tuples / n_diff_cells / loss_all / loss_tuples_mean / loss_cells_mean");
    if (x->pi && (!x->loss_w || !x->diff_w || !x->v_w)) return missing("with pi, loss_w / diff_w / v_w");

    a.agents = x->agents; a.max_sweeps = x->max_sweeps;
    a.noise_prob = x->noise_prob; a.eval_tol = x->eval_tol;
    tuple_strides(c, a.n_actions, a.tstride);
    for (int i = 0; i < N; i++) a.gamma[i] = x->gamma[i];
    a.noise_prob_g = x->noise_prob_g; a.sweep_gamma = x->sweep_gamma;
    a.tuple_policy = x->tuple_policy; a.cell_policy = x->cell_policy; a.reward = x->reward;
    a.band_lo = x->band_lo; a.band = x->band; a.noise_reward = x->noise_reward; a.pi = x->pi;
    a.iters = x->iters; a.sweeps = x->sweeps; a.n_diff_tuples = x->n_diff_tuples; a.n_diff_cells = x->n_diff_cells;
    a.loss_all = x->loss_all; a.loss_tuples_mean = x->loss_tuples_mean; a.loss_cells_mean = x->loss_cells_mean;
    a.loss_w = x->loss_w; a.diff_w = x->diff_w; a.v_w = x->v_w;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    if (lds_cu > 0 && a.lds_bytes > lds_cu) return lds_refusal("thrl_tuple_equilibrium_noise", need, N, x->n_cells);
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTenMaxBlocksPerCu, a.G);
    const int e = thrl::launch_tuple_equilibrium_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_tuple_equilibrium_noise launch") : THRL_OK;
}

int thrl_tuple_deviation_noise(const thrl_cfg* c, const thrl_tuple_deviation_noise_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_tuple_stationary's checks in its order, with the deviation and its rows as thrl_deviation_noise checks them;
    // every host-visible argument is checked before the device is touched
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags != 0) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_deviator(c, x->deviator, x->dev_len, x->n_steps)) != THRL_OK) return rc;
    if ((rc = check_dev_action(c, x->deviator, x->dev_action)) != THRL_OK) return rc;
    if ((rc = check_rows(x->row_begin, x->row_count, x->n_steps)) != THRL_OK) return rc;
    if ((rc = check_cells_band(x->n_cells, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_tol(x->ret_tol, "ret_tol")) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_cell_limit("thrl_tuple_deviation_noise", x->n_cells)) != THRL_OK) return rc;
    TdnArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.J = x->n_cells; a.W = x->band_w;
    const int64_t need = thrl::tdn_layout(a);            // the working set of include/thrl.h
    if (need > THRL_TDN_MAX_LDS) return lds_refusal("thrl_tuple_deviation_noise", need, N, x->n_cells);
    if (!x->tuple_policy || !x->cell_policy || !x->reward || !x->scaled || !x->band_lo || !x->band || !x->noise_reward)
        return missing("tuple_policy / cell_policy / reward / scaled / band_lo / band / noise_reward");
    if (!x->weights) return missing("weights");
    if (!x->base_reward || !x->base_action || !x->dev_share || !x->gain || !x->gain_dev || !x->low || !x->low_step
        || !x->ret_step || !x->dist || !x->mass)
        return missing("base_reward / base_action / dev_share / gain / gain_dev / low / low_step / ret_step / dist / mass");

    a.d = x->deviator; a.L = x->dev_len; a.K = x->n_steps; a.dev_action = x->dev_action;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.noise_prob = x->noise_prob; a.ret_tol = x->ret_tol; a.gamma_d = c->gamma[x->deviator];
    tuple_strides(c, a.n_actions, a.tstride);
    a.noise_prob_g = x->noise_prob_g; a.sweep_gamma = x->sweep_gamma;
    a.tuple_policy = x->tuple_policy; a.cell_policy = x->cell_policy; a.reward = x->reward; a.scaled = x->scaled;
    a.band_lo = x->band_lo; a.band = x->band; a.noise_reward = x->noise_reward; a.weights = x->weights;
    a.base_reward = x->base_reward; a.base_action = x->base_action; a.dev_share = x->dev_share; a.gain = x->gain;
    a.gain_dev = x->gain_dev; a.low = x->low; a.low_step = x->low_step; a.ret_step = x->ret_step; a.dist = x->dist;
    a.mass = x->mass; a.reward_rows = x->reward_rows; a.action_rows = x->action_rows; a.dist_rows = x->dist_rows;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    if (lds_cu > 0 && a.lds_bytes > lds_cu) return lds_refusal("thrl_tuple_deviation_noise", need, N, x->n_cells);
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kTdnMaxBlocksPerCu, a.G);
    const int e = thrl::launch_tuple_deviation_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_tdn_chain launch") : THRL_OK;
}

int thrl_price_probs(const thrl_cfg* c, const thrl_price_probs_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->flags != 0) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if (x->n_prices < 1) return fail(THRL_ERR_BAD_CONFIG, "n_prices=%d must be >= 1", x->n_prices);
    if (x->n_prices > THRL_STAT_MAX_CELLS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_price_probs: n_prices=%d, at most %d", x->n_prices, THRL_STAT_MAX_CELLS);
    if (!x->price) return fail(THRL_ERR_NULL, "price is NULL");
    for (int i = 0; i < c->n_agents; i++)
        if (x->kind[i] != 0 && (!x->nn_params[i] || !x->prob[i]))
            return fail(THRL_ERR_NULL, "nn_params[%d] / prob[%d] is NULL", i, i);
    for (int i = 0; i < c->n_agents; i++) {
        if (x->kind[i] == 0) continue;
        const int A = c->n_actions[i];
        const int P = x->kind[i] == 2 ? (int)thrl_ac_param_count(A) : (int)thrl_nn_param_count(A);
        const int e = thrl::launch_tp_probs(x->n_games, A, x->n_prices, x->nn_params[i], P, x->price, x->prob[i],
                                            (hipStream_t)stream);
        if (e) return hip_fail(e, "k_tp_probs launch");
    }
    return THRL_OK;
}

}  // extern "C"

// ---- what the six calls on sampled play share (the two chains, the two response calls, the two deviation tests); X is the
// call's public argument struct
namespace {

// the head of SpArgs: the counts, the tuple strides and the agents' kinds, epsilons and rows at the distinct prices
template <typename X>
void sp_fill_head(SpArgs& sa, const thrl_cfg* c, const X* x) {
    sa.G = x->n_games; sa.N = c->n_agents; sa.T = x->n_tuples; sa.D = x->n_prices;
    tuple_strides(c, sa.n_actions, sa.tstride);
    for (int i = 0; i < sa.N; i++) { sa.kind[i] = x->kind[i]; sa.eps[i] = x->eps[i]; sa.prob[i] = x->prob[i]; }
}

// the plan's tail: the device's figures, then *grid; where a block's LDS is more than the device's lds_cu, what
// refuse(lds_cu) returns: the refusal in the call's own words
template <typename R>
int sp_plan_grid(const SpArgs& sa, int max_per_cu, int* grid, R refuse) {
    int cus = 0, lds_cu = 0;
    if (const int rc = cu_figures(&cus, &lds_cu)) return rc;
    if (lds_cu > 0 && sa.lds_bytes > lds_cu) return refuse(lds_cu);
    *grid = grid_for(cus, lds_cu, sa.lds_bytes, max_per_cu, sa.G);
    return THRL_OK;
}

// the host-visible checks of both response calls behind their games, flags and reserved words (whose refusals an entry
// point words itself): thrl_sampled_chain's in its order, with the agents and their gammas as
// thrl_tuple_equilibrium_noise checks them; after_prices() is the place of the noise call's check of its nodes and band
template <typename X, typename M>
int sr_check_args(const thrl_cfg* c, const X* x, M after_prices) {
    const int N = c->n_agents;
    int rc;
    if ((rc = check_agents_mask(x->agents, N)) != THRL_OK) return rc;
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_prices(x->n_prices, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = after_prices()) != THRL_OK) return rc;
    if (!x->sweep_gamma && (rc = check_gamma(x->gamma, N, x->agents)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_sweeps, x->eval_tol, "max_sweeps", "eval_tol")) != THRL_OK) return rc;
    if (!x->eps_g && (rc = check_eps(N, x->kind, x->eps)) != THRL_OK) return rc;
    return THRL_OK;
}

// what both response calls hand to their kernels under one name: the agents, their gammas and the sweeps' limits, the
// noise-free inputs, pi and the eleven outputs; A is SrArgs or SrnArgs
template <typename A, typename X>
void sr_copy_common(A& a, const X* x) {
    for (int i = 0; i < a.sp.N; i++) a.gamma[i] = x->gamma[i];
    a.agents = x->agents; a.max_sweeps = x->max_sweeps; a.eval_tol = x->eval_tol;
    a.sp.eps_g = x->eps_g; a.sp.dpolicy = x->dpolicy; a.sp.grp_first = x->grp_first; a.sp.grp_perm = x->grp_perm;
    a.sp.reward = x->reward;
    a.sweep_gamma = x->sweep_gamma; a.pi = x->pi;
    a.iters = x->iters; a.sweeps = x->sweeps; a.loss_all = x->loss_all;
    a.loss_w = x->loss_w; a.gain_w = x->gain_w; a.v_w = x->v_w; a.br_prob_w = x->br_prob_w;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
}

// the host-visible checks of both deviation tests behind their games, flags and reserved words (whose refusals an entry
// point words itself): thrl_sampled_chain's in its order with the deviation and its rows as thrl_tuple_deviation_noise
// checks them; after_prices() is the place of the noise call's check of its nodes and band
template <typename X, typename M>
int sd_check_args(const thrl_cfg* c, const X* x, bool use_policy, M after_prices) {
    int rc;
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_prices(x->n_prices, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = after_prices()) != THRL_OK) return rc;
    if ((rc = check_deviator(c, x->deviator, x->dev_len, x->n_steps)) != THRL_OK) return rc;
    if (use_policy) {                                    // the strategy is dev_policy: no action of the deviator is one
        thrl_cfg none = *c;
        none.n_actions[x->deviator] = 0;
        if ((rc = check_dev_action(&none, x->deviator, x->dev_action)) != THRL_OK) return rc;
    } else if ((rc = check_dev_action(c, x->deviator, x->dev_action)) != THRL_OK) {
        return rc;
    }
    if ((rc = check_rows(x->row_begin, x->row_count, x->n_steps)) != THRL_OK) return rc;
    if ((rc = check_tol(x->ret_tol, "ret_tol")) != THRL_OK) return rc;
    if (!x->sweep_gamma) {                               // gamma in [0, 1]: both ends through the check of a tolerance
        if ((rc = check_tol(x->gamma, "gamma")) != THRL_OK) return rc;
        if ((rc = check_tol(1.0 - x->gamma, "1 - gamma")) != THRL_OK) return rc;
    }
    if (!x->eps_g && (rc = check_eps(c->n_agents, x->kind, x->eps)) != THRL_OK) return rc;
    return THRL_OK;
}

// the last NULL checks of both deviation tests (x_0, dev_policy under the call's flag, refused as missing(policy_names), and
// the eleven outputs), then what both hand to their kernels under one name: the noise-free tables into sa, the deviation, its
// rows and the outputs into a
template <typename X>
int sd_copy_common(thrl::SdArgs& a, SpArgs& sa, const X* x, bool use_policy, const char* policy_names) {
    if (!x->weights) return missing("weights");
    if (use_policy && !x->dev_policy) return missing(policy_names);
    if (!x->base_reward || !x->base_action || !x->base_price || !x->dev_share || !x->gain || !x->gain_dev || !x->low
        || !x->low_step || !x->ret_step || !x->dist || !x->mass)
        return missing("base_reward / base_action / base_price / dev_share / gain / gain_dev / low / low_step / ret_step / "
                       "dist / mass");
    sa.eps_g = x->eps_g; sa.dpolicy = x->dpolicy; sa.grp_first = x->grp_first; sa.grp_perm = x->grp_perm;
    sa.reward = x->reward; sa.scaled = x->scaled; sa.price = x->price;
    a.d = x->deviator; a.L = x->dev_len; a.K = x->n_steps; a.dev_action = x->dev_action; a.use_policy = use_policy;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.gamma = x->gamma; a.ret_tol = x->ret_tol;
    a.sweep_gamma = x->sweep_gamma; a.dev_policy = x->dev_policy; a.weights = x->weights;
    a.base_reward = x->base_reward; a.base_action = x->base_action; a.base_price = x->base_price;
    a.dev_share = x->dev_share; a.gain = x->gain; a.gain_dev = x->gain_dev; a.low = x->low; a.low_step = x->low_step;
    a.ret_step = x->ret_step; a.dist = x->dist; a.mass = x->mass;
    a.reward_rows = x->reward_rows; a.action_rows = x->action_rows; a.price_rows = x->price_rows; a.dist_rows = x->dist_rows;
    return THRL_OK;
}

}  // namespace

extern "C" {

int thrl_sampled_chain(const thrl_cfg* c, const thrl_sampled_chain_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked before the device is touched
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags & ~THRL_SP_START_TUPLE) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_prices(x->n_prices, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_iters, x->tol)) != THRL_OK) return rc;
    if (!x->eps_g && (rc = check_eps(N, x->kind, x->eps)) != THRL_OK) return rc;
    SpArgs a;
    memset(&a, 0, sizeof(a));
    sp_fill_head(a, c, x);
    a.max_iters = x->max_iters; a.start_tuple = (x->flags & THRL_SP_START_TUPLE) != 0;
    a.tol = x->tol;
    thrl::sp_layout(a);                              // the working set of include/thrl.h
    if (a.lds_bytes > THRL_SP_MAX_LDS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_chain: %d bytes of LDS per game (T=%d, n_prices=%d), at most %d",
                    a.lds_bytes, a.T, a.D, THRL_SP_MAX_LDS);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && !x->prob[i]) return fail(THRL_ERR_NULL, "prob[%d] is NULL", i);
    if (!x->dpolicy || !x->grp_first || !x->grp_perm || !x->reward || !x->scaled || !x->price)
        return fail(THRL_ERR_NULL, "dpolicy / grp_first / grp_perm / reward / scaled / price is NULL");
    if (!x->iters || !x->change || !x->mass || !x->samp_reward || !x->samp_action || !x->samp_price || !x->agree)
        return fail(THRL_ERR_NULL, "iters / change / mass / samp_reward / samp_action / samp_price / agree is NULL");
    if (a.start_tuple && !x->start) return fail(THRL_ERR_NULL, "start is NULL with THRL_SP_START_TUPLE");
    a.eps_g = x->eps_g; a.start = x->start; a.dpolicy = x->dpolicy; a.grp_first = x->grp_first; a.grp_perm = x->grp_perm;
    a.reward = x->reward; a.scaled = x->scaled; a.price = x->price;
    a.iters = x->iters; a.change = x->change; a.mass = x->mass; a.samp_reward = x->samp_reward;
    a.samp_action = x->samp_action; a.samp_price = x->samp_price; a.agree = x->agree; a.pi = x->pi;
    int grid = 0;
    rc = sp_plan_grid(a, kSpMaxBlocksPerCu, &grid, [&](int lds_cu) {
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_chain: %d bytes of LDS per game (T=%d, n_prices=%d), the device has %d",
                    a.lds_bytes, a.T, a.D, lds_cu);
    });
    if (rc) return rc;
    const int e = thrl::launch_sampled_chain(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_sp_chain launch") : THRL_OK;
}

int thrl_sampled_noise_chain(const thrl_cfg* c, const thrl_sampled_noise_chain_args* x, void* stream) {
    static_assert(THRL_SPN_TILE == thrl::kSpnTile, "include/thrl.h and thrl_sampled_noise.h disagree on the tile");
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked, and the working set planned, before any pointer is looked at
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags & ~(THRL_SPN_START_TUPLE | THRL_SPN_START_RESET)) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((x->flags & THRL_SPN_START_TUPLE) && (x->flags & THRL_SPN_START_RESET))
        return fail(THRL_ERR_BAD_CONFIG, "THRL_SPN_START_TUPLE and THRL_SPN_START_RESET are both set");
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_prices(x->n_prices, x->n_tuples)) != THRL_OK) return rc;
    if ((rc = check_nodes_band(x->n_nodes, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_iters, x->tol)) != THRL_OK) return rc;
    if (!x->eps_g && (rc = check_eps(N, x->kind, x->eps)) != THRL_OK) return rc;
    if ((rc = check_noise_prob_closed(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_node_limit("thrl_sampled_noise_chain", x->n_nodes)) != THRL_OK) return rc;
    thrl::SpnArgs a;
    memset(&a, 0, sizeof(a));
    SpArgs& sa = a.sp;
    sp_fill_head(sa, c, x);
    sa.max_iters = x->max_iters; sa.start_tuple = (x->flags & THRL_SPN_START_TUPLE) != 0;
    sa.tol = x->tol;
    a.Jn = x->n_nodes; a.W = x->band_w; a.start_reset = (x->flags & THRL_SPN_START_RESET) != 0;
    a.noise_prob = x->noise_prob;
    for (int i = 0; i < N; i++) a.nprob[i] = x->nprob[i];
    const int64_t lds = thrl::spn_layout(a);         // the working set of include/thrl.h
    if (lds > THRL_SP_MAX_LDS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_noise_chain: %lld bytes of LDS per game (T=%d, n_prices=%d, n_nodes=%d), at most %d",
                    (long long)lds, sa.T, sa.D, a.Jn, THRL_SP_MAX_LDS);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && (!x->prob[i] || !x->nprob[i])) return missing_rows(i);
    if (!x->dpolicy || !x->npolicy || !x->grp_first || !x->grp_perm || !x->reward || !x->scaled || !x->price)
        return fail(THRL_ERR_NULL, "dpolicy / npolicy / grp_first / grp_perm / reward / scaled / price is NULL");
    if (!x->band_lo || !x->band || !x->noise_price || !x->noise_reward || !x->node_w)
        return fail(THRL_ERR_NULL, "band_lo / band / noise_price / noise_reward / node_w is NULL");
    if (!x->iters || !x->change || !x->mass || !x->samp_reward || !x->samp_action || !x->samp_price || !x->agree)
        return fail(THRL_ERR_NULL, "iters / change / mass / samp_reward / samp_action / samp_price / agree is NULL");
    if (sa.start_tuple && !x->start) return fail(THRL_ERR_NULL, "start is NULL with THRL_SPN_START_TUPLE");
    sa.eps_g = x->eps_g; sa.start = x->start; sa.dpolicy = x->dpolicy; sa.grp_first = x->grp_first; sa.grp_perm = x->grp_perm;
    sa.reward = x->reward; sa.scaled = x->scaled; sa.price = x->price;
    sa.iters = x->iters; sa.change = x->change; sa.mass = x->mass; sa.samp_reward = x->samp_reward;
    sa.samp_action = x->samp_action; sa.samp_price = x->samp_price; sa.agree = x->agree; sa.pi = x->pi;
    a.noise_prob_g = x->noise_prob_g; a.npolicy = x->npolicy; a.band_lo = x->band_lo; a.band = x->band;
    a.noise_price = x->noise_price; a.noise_reward = x->noise_reward; a.node_w = x->node_w; a.max_jump = x->max_jump;
    int grid = 0;
    rc = sp_plan_grid(sa, kSpMaxBlocksPerCu, &grid, [&](int lds_cu) {
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_noise_chain: %d bytes of LDS per game (T=%d, n_prices=%d, n_nodes=%d), the device has %d",
                    sa.lds_bytes, sa.T, sa.D, a.Jn, lds_cu);
    });
    if (rc) return rc;
    const int e = thrl::launch_sampled_noise_chain(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_spn_jump / k_spn_chain launch") : THRL_OK;
}

int thrl_sampled_response(const thrl_cfg* c, const thrl_sampled_response_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked, and the working set planned, before any pointer is looked at
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags != 0) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    for (int k = 0; k < 2; k++)
        if (x->reserved[k] != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved[k]);
    if ((rc = sr_check_args(c, x, [] { return (int)THRL_OK; })) != THRL_OK) return rc;
    thrl::SrArgs a;
    memset(&a, 0, sizeof(a));
    SpArgs& sa = a.sp;
    sp_fill_head(sa, c, x);
    const int64_t lds = thrl::sr_layout(a);          // the working set of include/thrl_response.h
    // (the cells of this analysis are the distinct prices)
    if (lds > THRL_SR_MAX_LDS) return lds_refusal("thrl_sampled_response", lds, N, x->n_prices);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && !x->prob[i]) return fail(THRL_ERR_NULL, "prob[%d] is NULL", i);
    if (!x->dpolicy || !x->grp_first || !x->grp_perm || !x->reward) return missing("dpolicy / grp_first / grp_perm / reward");
    if (!x->iters || !x->sweeps || !x->n_diff || !x->loss_all || !x->loss_mean)
        return missing("iters / sweeps / n_diff / loss_all / loss_mean");
    if (x->pi && (!x->loss_w || !x->gain_w || !x->v_w || !x->br_prob_w)) return missing("with pi, loss_w / gain_w / v_w / br_prob_w");
    sr_copy_common(a, x);
    a.n_diff = x->n_diff; a.loss_mean = x->loss_mean;
    int grid = 0;
    rc = sp_plan_grid(sa, kSrMaxBlocksPerCu, &grid, [&](int) { return lds_refusal("thrl_sampled_response", lds, N, x->n_prices); });
    if (rc) return rc;
    const int e = thrl::launch_sampled_response(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_sr_response launch") : THRL_OK;
}

int thrl_sampled_response_noise(const thrl_cfg* c, const thrl_sampled_response_noise_args* x, void* stream) {
    static_assert(THRL_SRN_MAX_LDS == THRL_SR_MAX_LDS, "both response calls plan for a CU's LDS");
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_sampled_response's checks in its order with thrl_sampled_noise_chain's of the nodes and the noise between them;
    // every host-visible argument is checked, and the working set planned, before any pointer is looked at
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags != 0) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    for (int k = 0; k < 2; k++)
        if (x->reserved[k] != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved[k]);
    if ((rc = sr_check_args(c, x, [&] { return check_nodes_band(x->n_nodes, x->band_w); })) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_node_limit("thrl_sampled_response_noise", x->n_nodes)) != THRL_OK) return rc;
    thrl::SrnArgs a;
    memset(&a, 0, sizeof(a));
    SpArgs& sa = a.sp;
    sp_fill_head(sa, c, x);
    a.Jn = x->n_nodes; a.W = x->band_w;
    for (int i = 0; i < N; i++) a.nprob[i] = x->nprob[i];
    const int64_t lds = thrl::srn_layout(a);         // the working set of include/thrl_response_noise.h
    // (the cells of this analysis are its states: the distinct prices and the nodes)
    if (lds > THRL_SRN_MAX_LDS) return lds_refusal("thrl_sampled_response_noise", lds, N, x->n_prices + x->n_nodes);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && (!x->prob[i] || !x->nprob[i])) return missing_rows(i);
    if (!x->dpolicy || !x->npolicy || !x->grp_first || !x->grp_perm || !x->reward || !x->band_lo || !x->band || !x->noise_reward)
        return missing("dpolicy / npolicy / grp_first / grp_perm / reward / band_lo / band / noise_reward");
    if (!x->iters || !x->sweeps || !x->n_diff_prices || !x->n_diff_nodes || !x->loss_all || !x->loss_prices_mean
        || !x->loss_nodes_mean)
        return missing("iters / sweeps / n_diff_prices / n_diff_nodes / loss_all / loss_prices_mean / loss_nodes_mean");
    if (x->pi && (!x->loss_w || !x->gain_w || !x->v_w || !x->br_prob_w)) return missing("with pi, loss_w / gain_w / v_w / br_prob_w");
    sr_copy_common(a, x);
    a.noise_prob = x->noise_prob; a.noise_prob_g = x->noise_prob_g;
    a.npolicy = x->npolicy; a.band_lo = x->band_lo; a.band = x->band; a.noise_reward = x->noise_reward;
    a.n_diff_prices = x->n_diff_prices; a.n_diff_nodes = x->n_diff_nodes;
    a.loss_prices_mean = x->loss_prices_mean; a.loss_nodes_mean = x->loss_nodes_mean;
    int grid = 0;
    rc = sp_plan_grid(sa, kSrnMaxBlocksPerCu, &grid,
                      [&](int) { return lds_refusal("thrl_sampled_response_noise", lds, N, x->n_prices + x->n_nodes); });
    if (rc) return rc;
    const int e = thrl::launch_sampled_response_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_srn_response launch") : THRL_OK;
}

int thrl_sampled_deviation(const thrl_cfg* c, const thrl_sampled_deviation_args* x, void* stream) {
    static_assert(THRL_SD_MAX_LDS == THRL_SP_MAX_LDS, "the deviation test plans for a CU's LDS as sampled play does");
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_sampled_chain's checks in its order with the deviation and its rows as thrl_tuple_deviation_noise checks them;
    // every host-visible argument is checked, and the working set planned, before any pointer is looked at
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags & ~THRL_SD_POLICY) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    for (int k = 0; k < 2; k++)
        if (x->reserved[k] != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved[k]);
    const bool use_policy = (x->flags & THRL_SD_POLICY) != 0;
    if ((rc = sd_check_args(c, x, use_policy, [] { return (int)THRL_OK; })) != THRL_OK) return rc;
    thrl::SdArgs a;
    memset(&a, 0, sizeof(a));
    SpArgs& sa = a.sp;
    sp_fill_head(sa, c, x);
    const int64_t lds = thrl::sd_layout(a);          // the working set of include/thrl_sampled_deviation.h
    // (the cells of this analysis are the distinct prices)
    if (lds > THRL_SD_MAX_LDS) return lds_refusal("thrl_sampled_deviation", lds, N, x->n_prices);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && !x->prob[i]) return fail(THRL_ERR_NULL, "prob[%d] is NULL", i);
    if (!x->dpolicy || !x->grp_first || !x->grp_perm || !x->reward || !x->scaled || !x->price)
        return missing("dpolicy / grp_first / grp_perm / reward / scaled / price");
    if ((rc = sd_copy_common(a, sa, x, use_policy, "with THRL_SD_POLICY, dev_policy")) != THRL_OK) return rc;
    int grid = 0;
    rc = sp_plan_grid(sa, kSdMaxBlocksPerCu, &grid, [&](int) { return lds_refusal("thrl_sampled_deviation", lds, N, x->n_prices); });
    if (rc) return rc;
    const int e = thrl::launch_sampled_deviation(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_sd_chain launch") : THRL_OK;
}

int thrl_sampled_deviation_noise(const thrl_cfg* c, const thrl_sampled_deviation_noise_args* x, void* stream) {
    static_assert(THRL_SDN_MAX_LDS == THRL_SD_MAX_LDS && THRL_SDN_POLICY == THRL_SD_POLICY, "the two deviation tests of sampled play agree");
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_sampled_deviation's checks in its order with thrl_sampled_noise_chain's of the nodes and the noise between them;
    // every host-visible argument is checked, and the working set planned, before any pointer is looked at
    if ((rc = check_games(x->n_games)) != THRL_OK) return rc;
    if (x->flags & ~THRL_SDN_POLICY) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    for (int k = 0; k < 2; k++)
        if (x->reserved[k] != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved[k]);
    const bool use_policy = (x->flags & THRL_SDN_POLICY) != 0;
    if ((rc = sd_check_args(c, x, use_policy, [&] { return check_nodes_band(x->n_nodes, x->band_w); })) != THRL_OK) return rc;
    if ((rc = check_noise_prob_closed(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_node_limit("thrl_sampled_deviation_noise", x->n_nodes)) != THRL_OK) return rc;
    thrl::SdnArgs a;
    memset(&a, 0, sizeof(a));
    thrl::SpnArgs& na = a.n;
    SpArgs& sa = na.sp;
    thrl::SdArgs& sd = a.sd;
    sp_fill_head(sa, c, x);
    na.Jn = x->n_nodes; na.W = x->band_w; na.noise_prob = x->noise_prob;
    for (int i = 0; i < N; i++) na.nprob[i] = x->nprob[i];
    const int64_t lds = thrl::sdn_layout(a);         // the working set of include/thrl_sampled_deviation_noise.h
    // (the cells of this analysis are the deviator's states: the distinct prices and the nodes)
    if (lds > THRL_SDN_MAX_LDS) return lds_refusal("thrl_sampled_deviation_noise", lds, N, x->n_prices + x->n_nodes);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && (!x->prob[i] || !x->nprob[i])) return missing_rows(i);
    if (!x->dpolicy || !x->npolicy || !x->grp_first || !x->grp_perm || !x->reward || !x->scaled || !x->price)
        return missing("dpolicy / npolicy / grp_first / grp_perm / reward / scaled / price");
    if (!x->band_lo || !x->band || !x->noise_price || !x->noise_reward) return missing("band_lo / band / noise_price / noise_reward");
    if ((rc = sd_copy_common(sd, sa, x, use_policy, "with THRL_SDN_POLICY, dev_policy")) != THRL_OK) return rc;
    na.noise_prob_g = x->noise_prob_g; na.npolicy = x->npolicy; na.band_lo = x->band_lo; na.band = x->band;
    na.noise_price = x->noise_price; na.noise_reward = x->noise_reward;
    int grid = 0;
    rc = sp_plan_grid(sa, kSdnMaxBlocksPerCu, &grid,
                      [&](int) { return lds_refusal("thrl_sampled_deviation_noise", lds, N, x->n_prices + x->n_nodes); });
    if (rc) return rc;
    const int e = thrl::launch_sampled_deviation_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_sdn_chain launch") : THRL_OK;
}

}  // extern "C"

// ---- thrl_equilibrium: the per-config plan (tuple LUTs and state rows), built on the host and cached on the device
namespace {

struct EqKey {                      // everything of thrl_cfg the plan depends on, and the device it lives on
    int32_t dev, N;
    double env_a, env_b;
    int32_t n_states[THRL_MAXA], n_actions[THRL_MAXA];
    double max_state[THRL_MAXA], act_lo[THRL_MAXA], act_hi[THRL_MAXA];
};

struct EqHostPlan {
    int S = 0, T = 0;
    std::vector<double> rew;        // [N][T]
    std::vector<int32_t> srow;      // [N][S]
    std::vector<uint16_t> sid;      // [T]
};

struct EqSlot {
    bool used = false;
    EqKey key;
    int S = 0, T = 0;
    void* mem = nullptr;            // rew | srow | sid
    size_t off_srow = 0, off_sid = 0;
};

constexpr int kEqSlots = 4;
std::mutex g_eq_mu;
EqSlot g_eq_slot[kEqSlots];
int g_eq_next = 0;

EqKey eq_key(const thrl_cfg* c, int dev) {
    EqKey k;
    memset(&k, 0, sizeof(k));
    k.dev = dev; k.N = c->n_agents; k.env_a = c->env_a; k.env_b = c->env_b;
    for (int i = 0; i < c->n_agents; i++) {
        k.n_states[i] = c->n_states[i]; k.n_actions[i] = c->n_actions[i];
        k.max_state[i] = c->max_state[i]; k.act_lo[i] = c->act_lo[i]; k.act_hi[i] = c->act_hi[i];
    }
    return k;
}

// THRL_OK, or THRL_ERR_UNSUPPORTED past the limits of include/thrl.h.  The arithmetic is the device's scale_action,
// env_step (no noise) and encode64, operation for operation.
int eq_host_plan(const thrl_cfg* c, EqHostPlan& h) {
    const int N = c->n_agents;
    int64_t T = 1;
    for (int i = 0; i < N; i++) {
        T *= c->n_actions[i];
        if (T > THRL_EQ_MAX_TUPLES)
            return fail(THRL_ERR_UNSUPPORTED, "thrl_equilibrium: more than %d action tuples (prod n_actions)",
                        THRL_EQ_MAX_TUPLES);
    }
    h.T = (int)T;
    h.rew.assign((size_t)N * T, 0.0);
    h.sid.assign((size_t)T, 0);
    const double ratio = c->env_a / c->env_b;
    std::map<std::vector<int32_t>, int> ids;
    std::vector<std::vector<int32_t>> rows;
    std::vector<int32_t> x((size_t)N);
    for (int t = 0; t < (int)T; t++) {
        double A[THRL_MAXA];
        double Q = 0.0;
        int rest = t;
        int act[THRL_MAXA];
        for (int i = N - 1; i >= 0; i--) { act[i] = rest % c->n_actions[i]; rest /= c->n_actions[i]; }
        for (int i = 0; i < N; i++) {
            A[i] = ratio * h_scale(act[i], c, i);
            Q = Q + A[i];
        }
        double p = c->env_a - c->env_b * Q;
        if (!(p > 0.0)) p = 0.0;
        for (int i = 0; i < N; i++) {
            h.rew[(size_t)i * T + t] = p * A[i];
            const int r = h_encode64(p, c, i);
            x[(size_t)i] = r < 0 ? 0 : (r > c->n_states[i] ? c->n_states[i] : r);
        }
        auto it = ids.find(x);
        if (it == ids.end()) {
            if ((int)rows.size() == THRL_EQ_MAX_STATES)
                return fail(THRL_ERR_UNSUPPORTED, "thrl_equilibrium: more than %d distinct row tuples (states)",
                            THRL_EQ_MAX_STATES);
            it = ids.emplace(x, (int)rows.size()).first;
            rows.push_back(x);
        }
        h.sid[(size_t)t] = (uint16_t)it->second;
    }
    h.S = (int)rows.size();
    h.srow.assign((size_t)N * h.S, 0);
    for (int s = 0; s < h.S; s++)
        for (int i = 0; i < N; i++) h.srow[(size_t)i * h.S + s] = rows[(size_t)s][(size_t)i];
    return THRL_OK;
}

// The device copy of the plan for (cfg, current device): cached, at most kEqSlots configs, the oldest evicted after
// the device has drained (a kernel of an earlier call may still read it).
int eq_device_plan(const thrl_cfg* c, const EqHostPlan& h, EqSlot& out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail((int)e, "hipGetDevice");
    const EqKey key = eq_key(c, dev);
    std::lock_guard<std::mutex> lock(g_eq_mu);
    for (int k = 0; k < kEqSlots; k++)
        if (g_eq_slot[k].used && !memcmp(&g_eq_slot[k].key, &key, sizeof(key))) { out = g_eq_slot[k]; return THRL_OK; }
    EqSlot& sl = g_eq_slot[g_eq_next];
    if (sl.used) {
        int cur = dev;
        if ((e = hipSetDevice(sl.key.dev)) != hipSuccess) return hip_fail((int)e, "hipSetDevice");
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipFree(sl.mem);
        hipError_t e2 = hipSetDevice(cur);
        sl.used = false;
        sl.mem = nullptr;
        if (e != hipSuccess) return hip_fail((int)e, "releasing a cached equilibrium plan");
        if (e2 != hipSuccess) return hip_fail((int)e2, "hipSetDevice");
    }
    const size_t b_rew = h.rew.size() * sizeof(double), b_srow = h.srow.size() * sizeof(int32_t),
                 b_sid = h.sid.size() * sizeof(uint16_t);
    sl.off_srow = b_rew;
    sl.off_sid = b_rew + b_srow;
    if ((e = hipMalloc(&sl.mem, b_rew + b_srow + b_sid)) != hipSuccess) return hip_fail((int)e, "hipMalloc (equilibrium plan)");
    unsigned char* m = (unsigned char*)sl.mem;
    e = hipMemcpy(m, h.rew.data(), b_rew, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m + sl.off_srow, h.srow.data(), b_srow, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m + sl.off_sid, h.sid.data(), b_sid, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(sl.mem);
        sl.mem = nullptr;
        return hip_fail((int)e, "hipMemcpy (equilibrium plan)");
    }
    sl.used = true; sl.key = key; sl.S = h.S; sl.T = h.T;
    g_eq_next = (g_eq_next + 1) % kEqSlots;
    out = sl;
    return THRL_OK;
}

// The plan of cfg on the current device without deriving it again when it is cached (thrl_attractors: one call per
// analysis, the same config every time): out.S / out.T are the plan's.  A miss derives it and uploads it.
int eq_cached_plan(const thrl_cfg* c, EqSlot& out) {
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail((int)e, "hipGetDevice");
    const EqKey key = eq_key(c, dev);
    {
        std::lock_guard<std::mutex> lock(g_eq_mu);
        for (int k = 0; k < kEqSlots; k++)
            if (g_eq_slot[k].used && !memcmp(&g_eq_slot[k].key, &key, sizeof(key))) { out = g_eq_slot[k]; return THRL_OK; }
    }
    EqHostPlan h;
    const int rc = eq_host_plan(c, h);
    return rc != THRL_OK ? rc : eq_device_plan(c, h, out);
}

}  // namespace

extern "C" {

int thrl_equilibrium(const thrl_cfg* c, const void* q, const thrl_equilibrium_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    EqHostPlan h;
    if ((rc = eq_host_plan(c, h)) != THRL_OK) return rc;
    if (x->n_states) *x->n_states = h.S;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if ((rc = check_agents_mask(x->agents, N)) != THRL_OK) return rc;
    if (!x->sweep_gamma && (rc = check_gamma(c, x->agents)) != THRL_OK) return rc;
    if (!q || !x->state0 || !x->mu || !x->lam || !x->iters || !x->n_diff_all || !x->n_diff_on || !x->loss_all
        || !x->loss_on || !x->loss_all_mean || !x->loss_on_mean || !x->v_on)
        return fail(THRL_ERR_NULL, "q / state0 / mu / lam / iters / n_diff_all / n_diff_on / loss_all / loss_on / "
                                   "loss_all_mean / loss_on_mean / v_on is NULL");
    EqSlot sl;
    if ((rc = eq_device_plan(c, h, sl)) != THRL_OK) return rc;
    EqArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.S = h.S; a.T = h.T; a.agents = x->agents;
    a.small = h.S <= 64;
    a.stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a.ag, nullptr);
    tuple_strides(c, nullptr, a.tstride);
    thrl::eq_layout(a);
    if (a.lds_bytes > kEqLdsBudget)         // cannot happen within the limits (62 KB at S = 1024, T = 4096, N = 8)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_equilibrium: %d bytes of LDS per game", a.lds_bytes);
    a.q = q; a.state0 = x->state0; a.sweep_gamma = x->sweep_gamma;
    a.rew = (const double*)sl.mem;
    a.srow = (const int32_t*)((const unsigned char*)sl.mem + sl.off_srow);
    a.sid = (const uint16_t*)((const unsigned char*)sl.mem + sl.off_sid);
    a.mu = x->mu; a.lam = x->lam; a.iters = x->iters; a.n_diff_all = x->n_diff_all; a.n_diff_on = x->n_diff_on;
    a.loss_all = x->loss_all; a.loss_on = x->loss_on; a.loss_all_mean = x->loss_all_mean;
    a.loss_on_mean = x->loss_on_mean; a.v_on = x->v_on;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kEqMaxBlocksPerCu, a.G);
    const int e = thrl::launch_equilibrium(a, c->q_dtype, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_equilibrium launch") : THRL_OK;
}

int thrl_attractors(const thrl_cfg* c, const void* q, const thrl_attractors_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // S without a device: the limits and *n_states are answered from the host plan when no GPU holds a cached one
    EqSlot sl;
    int devs = 0;
    const bool have_dev = hipGetDeviceCount(&devs) == hipSuccess && devs > 0;
    if (!have_dev) (void)hipGetLastError();
    int S = 0, T = 0;
    if (have_dev) {
        if ((rc = eq_cached_plan(c, sl)) != THRL_OK) return rc;
        S = sl.S; T = sl.T;
    } else {
        EqHostPlan h;
        if ((rc = eq_host_plan(c, h)) != THRL_OK) return rc;
        S = h.S; T = h.T;
    }
    if (x->n_states) *x->n_states = S;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->flags & ~THRL_ATTR_POLICY_GIVEN) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->n_starts < 0 || x->n_starts > THRL_ATTR_MAX_STARTS)
        return fail(THRL_ERR_BAD_CONFIG, "n_starts=%d out of [0,%d]", x->n_starts, THRL_ATTR_MAX_STARTS);
    const bool given = (x->flags & THRL_ATTR_POLICY_GIVEN) != 0;
    if (!x->state0 || !x->policy || !x->n_attr || !x->mu_max || !x->n_cycle_states || !x->rep || !x->lam || !x->basin
        || !x->cycle_reward || !x->cycle_action || !x->rep_x0 || !x->mu_x0 || !x->slot_x0)
        return fail(THRL_ERR_NULL, "state0 / policy / n_attr / mu_max / n_cycle_states / rep / lam / basin / cycle_reward / "
                                   "cycle_action / rep_x0 / mu_x0 / slot_x0 is NULL");
    if (x->n_starts > 0 && (!x->start_rows || !x->start_w || !x->reset_mass || !x->reset_mass_other || !x->reset_reward))
        return fail(THRL_ERR_NULL, "n_starts=%d: start_rows / start_w / reset_mass / reset_mass_other / reset_reward is NULL",
                    x->n_starts);
    if (!given && !q) return fail(THRL_ERR_NULL, "q is NULL without THRL_ATTR_POLICY_GIVEN");
    if (!have_dev) return hip_fail((int)hipErrorNoDevice, "thrl_attractors");

    AttrArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.S = S; a.T = T; a.J = x->n_starts;
    while ((1 << a.L) < S) a.L++;
    fill_agents(c, a.ag, nullptr);
    tuple_strides(c, nullptr, a.tstride);
    a.P = table_rows(a.ag, N, a.row_off, nullptr, nullptr);
    const int64_t fixed = thrl::attr_layout(a);
    if (fixed > kAttrLdsBudget)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_attractors: %lld bytes of LDS per game (N=%d, S=%d, T=%d)", (long long)fixed,
                    N, S, T);

    if (!given && (rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;

    a.policy = x->policy; a.state0 = x->state0;
    a.rew = (const double*)sl.mem;
    a.srow = (const int32_t*)((const unsigned char*)sl.mem + sl.off_srow);
    a.sid = (const uint16_t*)((const unsigned char*)sl.mem + sl.off_sid);
    a.start_rows = x->start_rows; a.start_w = x->start_w;
    a.n_attr = x->n_attr; a.mu_max = x->mu_max; a.n_cycle_states = x->n_cycle_states;
    a.rep = x->rep; a.lam = x->lam; a.basin = x->basin;
    a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action;
    a.rep_x0 = x->rep_x0; a.mu_x0 = x->mu_x0; a.slot_x0 = x->slot_x0;
    a.reset_mass = x->reset_mass; a.reset_mass_other = x->reset_mass_other; a.reset_reward = x->reset_reward;
    a.state_rep = x->state_rep; a.state_mu = x->state_mu;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kAttrMaxBlocksPerCu, a.G);
    const int e = thrl::launch_attractors(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_attractors launch") : THRL_OK;
}

int thrl_stationary(const thrl_cfg* c, const void* q, const thrl_stationary_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // T is the product of the action counts: the tuple limit and *n_tuples need no plan, and every host-visible
    // argument is checked before the device is touched (the plan is fetched, and cached, only by a call that launches)
    int T = 0;
    if ((rc = check_tuple_limit(c, "thrl_stationary", &T)) != THRL_OK) return rc;
    if (x->n_tuples) *x->n_tuples = T;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->flags & ~(THRL_STAT_POLICY_GIVEN | THRL_STAT_START_STATE))
        return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((rc = check_cells_band(x->n_cells, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_iters, x->tol)) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_cell_limit("thrl_stationary", x->n_cells)) != THRL_OK) return rc;
    // LDS of a block: the two iterates, the staging of the ordered sums and the tuple per cell must fit
    StatArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.J = x->n_cells;
    const int64_t need = thrl::stat_layout(a);
    if (need > kStatLdsBudget) return lds_refusal("thrl_stationary", need, N, x->n_cells);
    const bool given = (x->flags & THRL_STAT_POLICY_GIVEN) != 0;
    const bool start_state = (x->flags & THRL_STAT_START_STATE) != 0;
    if (!x->cell_rows || !x->cell_w || !x->det_cell || !x->band_lo || !x->band || !x->noise_reward || !x->noise_price)
        return missing("cell_rows / cell_w / det_cell / band_lo / band / noise_reward / noise_price");
    if (!x->policy || !x->iters || !x->change || !x->mass || !x->stat_reward || !x->stat_action || !x->stat_price)
        return missing("policy / iters / change / mass / stat_reward / stat_action / stat_price");
    if (start_state && !x->state0) return fail(THRL_ERR_NULL, "state0 is NULL with THRL_STAT_START_STATE");
    if (!given && !q) return missing_q("THRL_STAT_POLICY_GIVEN");

    a.G = x->n_games; a.T = T; a.W = x->band_w;
    a.max_iters = x->max_iters; a.start_state = start_state;
    a.noise_prob = x->noise_prob; a.tol = x->tol;
    fill_agents(c, a.ag, &a.env);
    tuple_strides(c, nullptr, a.tstride);
    a.P = table_rows(a.ag, N, a.row_off, nullptr, nullptr);
    int devs = 0;
    if (hipGetDeviceCount(&devs) != hipSuccess || devs <= 0) {
        (void)hipGetLastError();
        return hip_fail((int)hipErrorNoDevice, "thrl_stationary");
    }
    EqSlot sl;
    if ((rc = eq_cached_plan(c, sl)) != THRL_OK) return rc;

    if (!given && (rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;

    a.policy = x->policy; a.noise_prob_g = x->noise_prob_g; a.state0 = x->state0;
    a.rew = (const double*)sl.mem;
    a.cell_rows = x->cell_rows; a.cell_w = x->cell_w; a.det_cell = x->det_cell; a.band_lo = x->band_lo; a.band = x->band;
    a.noise_reward = x->noise_reward; a.noise_price = x->noise_price;
    a.iters = x->iters; a.change = x->change; a.mass = x->mass; a.stat_reward = x->stat_reward;
    a.stat_action = x->stat_action; a.stat_price = x->stat_price; a.pi = x->pi;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kStatMaxBlocksPerCu, a.G);
    const int e = thrl::launch_stationary(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_stationary launch") : THRL_OK;
}

int thrl_equilibrium_noise(const thrl_cfg* c, const void* q, const thrl_equilibrium_noise_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_stationary's checks in its order, with the agents and their gammas as thrl_equilibrium checks them
    int T = 0;
    if ((rc = check_tuple_limit(c, "thrl_equilibrium_noise", &T)) != THRL_OK) return rc;
    if (x->n_tuples) *x->n_tuples = T;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if ((rc = check_agents_mask(x->agents, N)) != THRL_OK) return rc;
    if (x->flags & ~THRL_EQN_POLICY_GIVEN) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (!x->sweep_gamma && (rc = check_gamma(c, x->agents)) != THRL_OK) return rc;
    if ((rc = check_cells_band(x->n_cells, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_iters_tol(x->max_sweeps, x->eval_tol, "max_sweeps", "eval_tol")) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_cell_limit("thrl_equilibrium_noise", x->n_cells)) != THRL_OK) return rc;
    EqnArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.J = x->n_cells; a.T = T;
    const int64_t need = thrl::eqn_layout(a);
    if (need > kEqnLdsBudget) return lds_refusal("thrl_equilibrium_noise", need, N, x->n_cells);
    const bool given = (x->flags & THRL_EQN_POLICY_GIVEN) != 0;
    if (!x->cell_rows || !x->det_cell || !x->band_lo || !x->band || !x->noise_reward)
        return missing("cell_rows / det_cell / band_lo / band / noise_reward");
    if (!x->policy || !x->iters || !x->sweeps || !x->n_diff_all || !x->loss_all || !x->loss_all_mean)
        return missing("policy / iters / sweeps / n_diff_all / loss_all / loss_all_mean");
    if (x->weights && (!x->loss_w || !x->diff_w || !x->v_w)) return missing("with weights, loss_w / diff_w / v_w");
    if (!given && !q) return missing_q("THRL_EQN_POLICY_GIVEN");

    a.G = x->n_games; a.W = x->band_w; a.agents = x->agents;
    a.max_sweeps = x->max_sweeps;
    a.noise_prob = x->noise_prob; a.eval_tol = x->eval_tol;
    fill_agents(c, a.ag, nullptr);
    tuple_strides(c, nullptr, a.tstride);
    a.P = table_rows(a.ag, N, a.row_off, nullptr, nullptr);
    int devs = 0;
    if (hipGetDeviceCount(&devs) != hipSuccess || devs <= 0) {
        (void)hipGetLastError();
        return hip_fail((int)hipErrorNoDevice, "thrl_equilibrium_noise");
    }
    EqSlot sl;
    if ((rc = eq_cached_plan(c, sl)) != THRL_OK) return rc;

    if (!given && (rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;

    a.policy = x->policy; a.noise_prob_g = x->noise_prob_g; a.sweep_gamma = x->sweep_gamma;
    a.rew = (const double*)sl.mem;
    a.cell_rows = x->cell_rows; a.det_cell = x->det_cell; a.band_lo = x->band_lo; a.band = x->band;
    a.noise_reward = x->noise_reward; a.weights = x->weights;
    a.iters = x->iters; a.sweeps = x->sweeps; a.n_diff_all = x->n_diff_all;
    a.loss_all = x->loss_all; a.loss_all_mean = x->loss_all_mean; a.loss_w = x->loss_w; a.diff_w = x->diff_w; a.v_w = x->v_w;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kEqnMaxBlocksPerCu, a.G);
    const int e = thrl::launch_equilibrium_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_equilibrium_noise launch") : THRL_OK;
}

int thrl_deviation_noise(const thrl_cfg* c, const void* q, const thrl_deviation_noise_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // thrl_stationary's checks in its order, with the deviation and its rows as thrl_deviation checks them
    int T = 0;
    if ((rc = check_tuple_limit(c, "thrl_deviation_noise", &T)) != THRL_OK) return rc;
    if (x->n_tuples) *x->n_tuples = T;
    if ((rc = check_games_of(x->n_games, c)) != THRL_OK) return rc;
    if (x->flags & ~THRL_STAT_POLICY_GIVEN) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((rc = check_deviator(c, x->deviator, x->dev_len, x->n_steps)) != THRL_OK) return rc;
    if ((rc = check_dev_action(c, x->deviator, x->dev_action)) != THRL_OK) return rc;
    if ((rc = check_rows(x->row_begin, x->row_count, x->n_steps)) != THRL_OK) return rc;
    if ((rc = check_cells_band(x->n_cells, x->band_w)) != THRL_OK) return rc;
    if ((rc = check_tol(x->ret_tol, "ret_tol")) != THRL_OK) return rc;
    if ((rc = check_noise_prob(x->noise_prob_g, x->noise_prob)) != THRL_OK) return rc;
    if ((rc = check_cell_limit("thrl_deviation_noise", x->n_cells)) != THRL_OK) return rc;
    DevnArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.J = x->n_cells;
    const int64_t need = thrl::devn_layout(a);
    if (need > kDevnLdsBudget) return lds_refusal("thrl_deviation_noise", need, N, x->n_cells);
    const bool given = (x->flags & THRL_STAT_POLICY_GIVEN) != 0;
    if (!x->cell_rows || !x->det_cell || !x->band_lo || !x->band || !x->noise_reward)
        return missing("cell_rows / det_cell / band_lo / band / noise_reward");
    if (!x->weights) return missing("weights");
    if (!x->policy || !x->base_reward || !x->base_action || !x->dev_share || !x->gain || !x->gain_dev || !x->low
        || !x->low_step || !x->ret_step || !x->dist || !x->mass)
        return missing("policy / base_reward / base_action / dev_share / gain / gain_dev / low / low_step / ret_step / dist / "
                       "mass");
    if (!given && !q) return missing_q("THRL_STAT_POLICY_GIVEN");

    a.G = x->n_games; a.T = T; a.W = x->band_w;
    a.d = x->deviator; a.L = x->dev_len; a.K = x->n_steps; a.dev_action = x->dev_action;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.noise_prob = x->noise_prob; a.ret_tol = x->ret_tol; a.gamma_d = c->gamma[x->deviator];
    fill_agents(c, a.ag, nullptr);
    tuple_strides(c, nullptr, a.tstride);
    a.P = table_rows(a.ag, N, a.row_off, nullptr, nullptr);
    int devs = 0;
    if (hipGetDeviceCount(&devs) != hipSuccess || devs <= 0) {
        (void)hipGetLastError();
        return hip_fail((int)hipErrorNoDevice, "thrl_deviation_noise");
    }
    EqSlot sl;
    if ((rc = eq_cached_plan(c, sl)) != THRL_OK) return rc;

    if (!given && (rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;

    a.policy = x->policy; a.noise_prob_g = x->noise_prob_g; a.sweep_gamma = x->sweep_gamma; a.weights = x->weights;
    a.rew = (const double*)sl.mem;
    a.cell_rows = x->cell_rows; a.det_cell = x->det_cell; a.band_lo = x->band_lo; a.band = x->band;
    a.noise_reward = x->noise_reward;
    a.base_reward = x->base_reward; a.base_action = x->base_action; a.dev_share = x->dev_share; a.gain = x->gain;
    a.gain_dev = x->gain_dev; a.low = x->low; a.low_step = x->low_step; a.ret_step = x->ret_step; a.dist = x->dist;
    a.mass = x->mass; a.reward_rows = x->reward_rows; a.action_rows = x->action_rows; a.dist_rows = x->dist_rows;
    int cus = 0, lds_cu = 0;
    if ((rc = cu_figures(&cus, &lds_cu)) != THRL_OK) return rc;
    const int grid = grid_for(cus, lds_cu, a.lds_bytes, kDevnMaxBlocksPerCu, a.G);
    const int e = thrl::launch_deviation_noise(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_deviation_noise launch") : THRL_OK;
}

}  // extern "C"
