// api_helpers_check.cpp -- a stand-alone host program over the shared planning code of the analysis entry points:
// the LDS layout functions of the analysis headers and the pure helpers of thrl_api_analysis.hip (which it includes,
// to reach its file-local helpers), on shapes up to the limits of include/thrl.h: T = 4096 tuples, S = 1024 states,
// N = 8 agents, 4096 cells.  tests/test_api_helpers_host.py builds it as host code with -fsanitize=address,undefined
// against libthrl_hip.so (fail(), validate(), reach_window() and the launch functions come from there) and runs it.
// It makes no HIP call: cu_figures() and the entry points themselves are not called.
#include "../th_rl_amd/csrc/thrl_api_analysis.hip"

#include <initializer_list>

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

static void aligned(std::initializer_list<int32_t> offs, int to, int32_t lds_bytes) {
    for (int32_t o : offs) CHECK(o >= 0 && o % to == 0 && o < lds_bytes);
}

constexpr int kCuLds = 160 * 1024;

static void layouts(int N, int T, int S, int J) {
    {   // thrl_tuple_equilibrium: the bound its header states
        TaEqArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.T = T;
        ta_eq_layout(a);
        aligned({a.o_va, a.o_vb, a.o_rew, a.o_misc}, 8, a.lds_bytes);
        aligned({a.o_na, a.o_nb, a.o_sigma, a.o_jn, a.o_mark, a.o_base}, 2, a.lds_bytes);
        CHECK(a.o_misc + kTaEqLdsFixed == a.lds_bytes);
        CHECK(a.lds_bytes <= kTaEqLdsPerTuple * T + kTaEqLdsFixed + 144 && a.lds_bytes <= kCuLds);
    }
    {   // thrl_tuple_attractors
        TatArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.T = T;
        while ((1 << a.L) < a.T) a.L++;
        tat_layout(a);
        aligned({a.o_cw, a.o_cprod, a.o_cmean}, 8, a.lds_bytes);
        aligned({a.o_basin, a.o_lamc, a.o_sel, a.o_red}, 4, a.lds_bytes);
        aligned({a.o_f, a.o_pa, a.o_pb, a.o_ma, a.o_mb, a.o_rep, a.o_on, a.o_slot, a.o_cslot}, 2, a.lds_bytes);
        CHECK(a.o_cslot + 2 * kTatBlock == a.lds_bytes);
        CHECK(a.lds_bytes <= kTatLdsPerTuple * T + (8 * (1 + N) + 2) * kTatBlock + 1024 + 16 * 10 && a.lds_bytes <= kCuLds);
    }
    {   // thrl_tuple_stationary
        TsArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.T = T; a.J = J;
        ts_layout(a);
        aligned({a.o_ma, a.o_mb, a.o_nu, a.o_prod}, 8, a.lds_bytes);
        aligned({a.o_permk, a.o_startk, a.o_permt, a.o_startt}, 2, a.lds_bytes);
        CHECK(a.o_nu == a.o_mb + 8 * T);                    // nu directly behind the second iterate
        CHECK(a.o_startt + 2 * (T + 1) <= a.lds_bytes && a.lds_bytes <= kCuLds);
    }
    {   // thrl_equilibrium: the wrapper refuses lds_bytes over the budget, which cannot happen within the limits
        EqArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.T = T; a.S = S;
        eq_layout(a);
        aligned({a.o_va, a.o_vb, a.o_vpi, a.o_rew}, 8, a.lds_bytes);
        aligned({a.o_base, a.o_x0row}, 4, a.lds_bytes);
        aligned({a.o_sid, a.o_first, a.o_pol, a.o_sigma, a.o_jn, a.o_na, a.o_nb}, 2, a.lds_bytes);
        CHECK(a.o_nb + 2 * S <= a.lds_bytes && a.lds_bytes <= kEqLdsBudget);
        CHECK(a.lut_lds == (a.o_base - a.o_rew == 8 * N * T));
    }
    {   // thrl_attractors: the wrapper refuses the returned bytes over the budget (at S = 1024 with N = 8 it does)
        AttrArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.T = T; a.S = S;
        while ((1 << a.L) < S) a.L++;
        const int64_t fixed = attr_layout(a);
        aligned({a.o_rew, a.o_cw, a.o_cprod}, 8, a.lds_bytes);
        aligned({a.o_basin, a.o_lamc, a.o_x0row, a.o_sel, a.o_cslot}, 4, a.lds_bytes);
        aligned({a.o_sid, a.o_pol, a.o_lev, a.o_ma, a.o_mb, a.o_rep, a.o_mu, a.o_on, a.o_tup, a.o_slot}, 2, a.lds_bytes);
        CHECK(a.o_slot + 2 * S <= a.lds_bytes);
        CHECK(a.lds_bytes <= fixed + (a.lut_lds ? 8 * (int64_t)N * T : 0));
        if (fixed <= kAttrLdsBudget) CHECK(a.lds_bytes <= kAttrLdsBudget);
    }
    {   // thrl_stationary: the wrapper refuses the returned bytes over the budget (at 4096 cells it does)
        StatArgs a;
        memset(&a, 0, sizeof(a));
        a.N = N; a.J = J;
        const int64_t need = stat_layout(a);
        aligned({a.o_mua, a.o_mub, a.o_prod}, 8, a.lds_bytes);
        aligned({a.o_boff, a.o_blo}, 4, a.lds_bytes);
        aligned({a.o_det, a.o_tup}, 2, a.lds_bytes);
        CHECK(a.o_tup + 2 * J <= a.lds_bytes);
        CHECK(a.lds_bytes <= need + (a.cell_lds ? 10 * (int64_t)J : 0));
        if (need <= kStatLdsBudget) CHECK(a.lds_bytes <= kStatLdsBudget);
    }
}

static thrl_cfg config(int N, const int* actions, int states) {
    thrl_cfg c;
    memset(&c, 0, sizeof(c));
    c.n_games = 64; c.n_agents = N; c.max_steps = 100; c.env_a = 10.0; c.env_b = 1.0;
    for (int i = 0; i < N; i++) {
        c.n_states[i] = states; c.n_actions[i] = actions[i]; c.max_state[i] = 25.0;
        c.act_lo[i] = 0.2 / N; c.act_hi[i] = 0.4 / N; c.gamma[i] = 0.95; c.alpha[i] = 0.1;
    }
    return c;
}

static bool refused(int rc, int code, const char* text) {
    return rc == code && strstr(thrl_last_error(), text) != nullptr;
}

int main() {
    for (int N : {1, 2, 3, 8})
        for (int T : {1, 2, 12, 441, 4095, 4096})
            for (int S : {1, 41, 64, 65, 1023, 1024})
                for (int J : {1, 2, 101, 3001, 4096}) layouts(N, T, S, J);

    // eight agents, 4096 tuples, the largest state grid
    const int actions[THRL_MAXA] = {2, 2, 2, 2, 2, 2, 8, 8};
    const thrl_cfg c = config(THRL_MAXA, actions, 32000);
    CHECK(validate(&c) == THRL_OK);
    int32_t n_actions[THRL_MAXA], tstride[THRL_MAXA], only[THRL_MAXA];
    tuple_strides(&c, n_actions, tstride);
    tuple_strides(&c, nullptr, only);
    CHECK(tstride[THRL_MAXA - 1] == 1 && tstride[0] * n_actions[0] == THRL_TP_MAX_TUPLES);
    for (int i = 0; i < THRL_MAXA; i++) CHECK(n_actions[i] == actions[i] && only[i] == tstride[i]);
    for (int i = 0; i + 1 < THRL_MAXA; i++) CHECK(tstride[i] == tstride[i + 1] * n_actions[i + 1]);

    AgentParams ag[THRL_MAXA];
    fill_agents(&c, ag, nullptr);
    int32_t row_off[THRL_MAXA + 1], table_off[THRL_MAXA], na[THRL_MAXA], bare[THRL_MAXA];
    const int P = table_rows(ag, THRL_MAXA, row_off, table_off, na);
    CHECK(P == THRL_MAXA * 32001 && table_rows(ag, THRL_MAXA, bare, nullptr, nullptr) == P);
    for (int i = 0; i < THRL_MAXA; i++)
        CHECK(row_off[i] == i * 32001 && bare[i] == row_off[i] && table_off[i] == ag[i].table_off && na[i] == actions[i]);
    CHECK((size_t)table_off[THRL_MAXA - 1] + (size_t)32001 * 8 == thrl_table_stride(&c));

    int32_t win_lo[THRL_MAXA], win_n[THRL_MAXA], pol_off[THRL_MAXA + 1], lut_off[THRL_MAXA], entries = -1, lut_n = -1;
    reach_tables(&c, win_lo, win_n, pol_off, lut_off, &entries, &lut_n);
    CHECK(lut_n == 28 && pol_off[THRL_MAXA] == entries && pol_off[0] == 0 && lut_off[0] == 0);
    for (int i = 0; i < THRL_MAXA; i++) {
        CHECK(win_lo[i] >= 0 && win_n[i] >= 1 && win_lo[i] + win_n[i] <= 32001);
        CHECK(pol_off[i + 1] == pol_off[i] + win_n[i] + 1);
        if (i) CHECK(lut_off[i] == lut_off[i - 1] + actions[i - 1]);
    }

    // the staged window: 16-byte chunks at both ends of the game's block, or nothing
    const int small[2] = {21, 21};
    thrl_cfg c2 = config(2, small, 100);
    alignas(16) static char q[32];
    int32_t staged = -1;
    CHECK(staged_window(&c2, q, 64 * 1024, &staged) == ((2 * 101 * 21 + 8) * 4 + 15) / 16 * 16 && staged == 1);
    CHECK(staged_window(&c2, q + 4, 64 * 1024, &staged) == 0 && staged == 0);          // q not 16-byte aligned
    CHECK(staged_window(&c2, q, 1024, &staged) == 0 && staged == 0);                   // over the budget
    c2.q_dtype = 1;
    CHECK(staged_window(&c2, q, 64 * 1024, &staged) == ((2 * 101 * 21 + 4) * 8 + 15) / 16 * 16 && staged == 1);
    CHECK(staged_window(&c, q, 64 * 1024, &staged) == 0 && staged == 0);               // 8 x 32001 rows

    // grids: per CU what LDS allows, at most the cap, at least one, never more blocks than games
    CHECK(grid_for(256, kCuLds, 0, 16, 1 << 30) == 256 * 16);                          // no LDS: the cap
    CHECK(grid_for(256, kCuLds, 64 * 1024, 16, 1 << 30) == 256 * 2);
    CHECK(grid_for(256, kCuLds, 4096, 16, 1 << 30) == 256 * 16);
    CHECK(grid_for(256, kCuLds, kCuLds + 1, 16, 1 << 30) == 256);                      // the zero quotient clamps to one
    CHECK(grid_for(256, 0, 64 * 1024, 7, 1 << 30) == 256 * 7);                         // unknown LDS per CU: the cap
    CHECK(grid_for(0, kCuLds, 4096, 4, 1 << 30) == 4);                                 // unknown CU count: one CU
    CHECK(grid_for(256, kCuLds, 4096, 32, 5) == 5 && grid_for(256, kCuLds, 4096, 32, 1) == 1);
    CHECK(grid_for(INT32_MAX, kCuLds, 16, 32, INT32_MAX) == INT32_MAX);                // the product is taken in 64 bits

    // the check helpers: THRL_OK inside the range, the refusal and its words outside
    CHECK(check_games_of(1, &c) == THRL_OK && check_games_of(64, &c) == THRL_OK);
    CHECK(refused(check_games_of(65, &c), THRL_ERR_BAD_CONFIG, "n_games=65 out of [1,64]"));
    CHECK(check_games(INT32_MAX) == THRL_OK && refused(check_games(0), THRL_ERR_BAD_CONFIG, "n_games=0 must be >= 1"));
    CHECK(check_horizon(THRL_DEV_MAX_HORIZON) == THRL_OK);
    CHECK(refused(check_horizon(THRL_DEV_MAX_HORIZON + 1), THRL_ERR_BAD_CONFIG, "horizon="));
    CHECK(check_rows(0, THRL_DEV_MAX_STEPS, THRL_DEV_MAX_STEPS) == THRL_OK);
    CHECK(refused(check_rows(INT32_MAX, INT32_MAX, THRL_DEV_MAX_STEPS), THRL_ERR_BAD_CONFIG, "rows ["));
    CHECK(check_steps_rows(0, 0, 0) == THRL_OK && check_steps_rows(THRL_DEV_MAX_STEPS, 1, 2) == THRL_OK);
    CHECK(refused(check_steps_rows(-1, 0, 0), THRL_ERR_BAD_CONFIG, "n_steps=-1 out of [0,"));
    CHECK(refused(check_steps_rows(4, 4, 1), THRL_ERR_BAD_CONFIG, "rows [4, 4 + 1)"));
    CHECK(check_deviation(&c, THRL_MAXA - 1, 1, THRL_DEV_MAX_STEPS, 1, 7) == THRL_OK);
    CHECK(check_deviation(&c, 0, 3, 3, THRL_DEV_MAX_HORIZON, -1) == THRL_OK);
    CHECK(refused(check_deviation(&c, THRL_MAXA, 1, 8, 1, -1), THRL_ERR_BAD_CONFIG, "deviator=8"));
    CHECK(refused(check_deviation(&c, 0, 0, 8, 1, -1), THRL_ERR_BAD_CONFIG, "dev_len=0"));
    CHECK(refused(check_deviation(&c, 0, 9, 8, 1, -1), THRL_ERR_BAD_CONFIG, "n_steps=8 out of [dev_len=9"));
    CHECK(refused(check_deviation(&c, 0, 1, 8, 0, -1), THRL_ERR_BAD_CONFIG, "horizon=0"));
    CHECK(refused(check_deviation(&c, 0, 1, 8, 1, 2), THRL_ERR_BAD_CONFIG, "dev_action=2"));
    CHECK(check_iters_tol(THRL_STAT_MAX_ITERS, 0.0) == THRL_OK);
    CHECK(refused(check_iters_tol(THRL_STAT_MAX_ITERS + 1, 0.0), THRL_ERR_BAD_CONFIG, "max_iters="));
    CHECK(refused(check_iters_tol(1, -1.0), THRL_ERR_BAD_CONFIG, "tol=-1"));
    const int32_t kind[THRL_MAXA] = {0, 1, 0, 2, 0, 0, 0, 0};
    double eps[THRL_MAXA] = {0.0, 7.0, 1.0, -3.0, 0.5, 0.5, 0.5, 0.5};                 // a network's epsilon is not read
    CHECK(check_eps(THRL_MAXA, kind, eps) == THRL_OK);
    eps[THRL_MAXA - 1] = 1.5;
    CHECK(refused(check_eps(THRL_MAXA, kind, eps), THRL_ERR_BAD_CONFIG, "eps[7]=1.5"));
    CHECK(check_agents_mask(0xff, THRL_MAXA) == THRL_OK && check_agents_mask(0x80, THRL_MAXA) == THRL_OK);
    CHECK(refused(check_agents_mask(0x100, THRL_MAXA), THRL_ERR_BAD_CONFIG, "agents=0x100"));
    CHECK(refused(check_agents_mask(0, THRL_MAXA), THRL_ERR_BAD_CONFIG, "agents=0x0"));
    thrl_cfg c3 = c;
    c3.gamma[THRL_MAXA - 1] = 1.0;
    CHECK(check_gamma(&c, 0xff) == THRL_OK && check_gamma(&c3, 0x7f) == THRL_OK);
    CHECK(refused(check_gamma(&c3, 0x80), THRL_ERR_BAD_CONFIG, "agent 7: gamma=1"));

    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("api helpers ok\n");
    return 0;
}
