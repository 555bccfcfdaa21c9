// solve_dev_check.cpp -- a stand-alone host program over the __host__ __device__ pieces of th_rl_amd/csrc/thrl_solve_dev.h,
// the ones the six kernels that solve a game's whole state graph share.  Every map F on n states for n = 1 .. 5 (3,413
// maps): the walk that marks first visits against find_cycle of thrl_walk_dev.h from every start (mu, lam, x_mu), and
// the doubling steps against a step-by-step walk (rep as the orbit minimum of the cycle, the on-cycle set; the value of
// a constant-reward policy against its closed form).  The band range against a count, every b0 around [0, J) and the
// two ends of int32.  The round count D against its definition, the relative loss on its three branches, the margin,
// the blend, the first maximum and the attractor key.  tests/test_solve_dev_host.py builds it as host code with
// -fsanitize=address,undefined and runs it.  It makes no HIP call.
#include "../th_rl_amd/csrc/thrl_solve_dev.h"
#include "../th_rl_amd/csrc/thrl_walk_dev.h"

#include <math.h>
#include <stdio.h>

using namespace thrl;

static int g_failed = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { if (g_failed < 20) printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

constexpr int kMaxStates = 5;

// mu, lam and x_mu of every start against the cycle search with a horizon that always finds the cycle
static void check_walk(const uint16_t* F, int n) {
    for (int x0 = 0; x0 < n; x0++) {
        int16_t first[kMaxStates];
        for (int k = 0; k < n; k++) first[k] = -1;
        int mu = -7, lam = -7;
        const int xmu = first_visit_walk(first, F, n, x0, 0, mu, lam);
        int rmu = -1, rlam = -1, rs = -1;
        const bool found = find_cycle(x0, 1, 2 * n, [&](int& x) { x = F[x]; }, rmu, rlam, rs, true);
        CHECK(found && mu == rmu && lam == rlam && xmu == rs);
        // started one step late, as k_equilibrium does when x_0 is no state: the steps count from 1
        for (int k = 0; k < n; k++) first[k] = -1;
        int mu1 = -7, lam1 = -7;
        const int xmu1 = first_visit_walk(first, F, n, F[x0], 1, mu1, lam1);
        int y = F[x0], ymu = -1, ylam = -1, ys = -1;
        find_cycle(y, 1, 2 * n, [&](int& x) { x = F[x]; }, ymu, ylam, ys, true);
        CHECK(mu1 == ymu + 1 && lam1 == ylam && xmu1 == ys);
    }
}

// L = ceil(log2 n) rounds of double_min: the image of p is the on-cycle set and m(p(s)) the least state of s's cycle;
// then the absorbed map's step count, as k_ta_attractors doubles it, is mu.  Against a walk of n steps and a brute force.
static void check_doubling(const uint16_t* F, int n) {
    int L = 0;
    while ((1 << L) < n) L++;
    uint16_t pa[kMaxStates], pb[kMaxStates], ma[kMaxStates], mb[kMaxStates];
    for (int s = 0; s < n; s++) { pa[s] = F[s]; ma[s] = (uint16_t)s; }
    uint16_t *po = pa, *pn = pb, *mo = ma, *mn = mb;
    for (int k = 0; k < L; k++) {
        for (int s = 0; s < n; s++) double_min(po, pn, mo, mn, s);
        uint16_t* t = po; po = pn; pn = t;
        t = mo; mo = mn; mn = t;
    }
    bool on[kMaxStates] = {false, false, false, false, false};
    for (int s = 0; s < n; s++) on[po[s]] = true;
    for (int s = 0; s < n; s++) {
        int x = s;                                      // brute force: n steps land on the cycle
        for (int j = 0; j < n; j++) x = F[x];
        int least = x, y = F[x], lam = 1;
        while (y != x) { if (y < least) least = y; y = F[y]; lam++; }
        bool cyc = false;                               // s is on a cycle iff it returns to itself
        y = s;
        for (int j = 0; j < n; j++) { y = F[y]; if (y == s) cyc = true; }
        int mu = 0;
        for (y = s; ; y = F[y], mu++) {
            bool c = false;
            int z = y;
            for (int j = 0; j < n; j++) { z = F[z]; if (z == y) c = true; }
            if (c) break;
        }
        CHECK(on[s] == cyc);
        CHECK(mo[po[s]] == least);
        (void)lam;
        // the absorbed step count of k_ta_attractors, doubled on the host the way the kernel does it
        uint16_t ha[kMaxStates], hb[kMaxStates], da[kMaxStates], db[kMaxStates];
        for (int u = 0; u < n; u++) { ha[u] = on[u] ? (uint16_t)u : F[u]; da[u] = on[u] ? 0 : 1; }
        uint16_t *ho = ha, *hn = hb, *dold = da, *dnew = db;
        for (int k = 0; k < L; k++) {
            for (int u = 0; u < n; u++) { const int m = ho[u]; hn[u] = ho[m]; dnew[u] = (uint16_t)(dold[u] + dold[m]); }
            uint16_t* t = ho; ho = hn; hn = t;
            t = dold; dold = dnew; dnew = t;
        }
        CHECK(dold[s] == mu);
    }
    // double_value with reward 1 everywhere: after D rounds V = sum of gam^k over 2^D terms, whatever the map
    const double gam = 0.5;
    const int D = doubling_rounds(gam);
    double Va[kMaxStates], Vb[kMaxStates];
    uint16_t na[kMaxStates], nb[kMaxStates];
    for (int s = 0; s < n; s++) { Va[s] = 1.0; na[s] = F[s]; }
    double *Vo = Va, *Vn = Vb, w = gam;
    uint16_t *no = na, *nn = nb;
    for (int d = 0; d < D; d++) {
        for (int s = 0; s < n; s++) double_value(Vo, Vn, no, nn, w, s);
        double* tv = Vo; Vo = Vn; Vn = tv;
        uint16_t* tn = no; no = nn; nn = tn;
        w = w * w;
    }
    for (int s = 0; s < n; s++) {
        CHECK(Vo[s] == 2.0);                            // 2 - 2^-31 after five rounds, exact; 2 - 2^-63 rounds to 2
        int x = s;                                      // n o n .. = F^(2^D); 2^D = 128 steps by hand
        for (int j = 0; j < (1 << D); j++) x = F[x];
        CHECK(no[s] == x);
    }
}

static void check_band() {
    const int edge[2] = {INT32_MIN, INT32_MAX};
    for (int W = 0; W <= 6; W++)
        for (int J = 1; J <= 6; J++) {
            const auto one = [&](int b0) {
                int count = 0, lo = -1, hi = -1;
                for (int w = 0; w < W; w++) {
                    const int64_t c = (int64_t)b0 + w;
                    if (c >= 0 && c < J) { if (!count) lo = w; hi = w + 1; count++; }
                }
                const int w0 = band_first(b0, W), w1 = band_end(b0, W, J);
                CHECK(w0 >= 0 && w0 <= W && w1 >= 0 && w1 <= W);
                CHECK((w1 > w0 ? w1 - w0 : 0) == count);
                if (count) CHECK(w0 == lo && w1 == hi);
                CHECK(count <= J);
            };
            for (int b0 = -2 * W - 2; b0 <= J + 2; b0++) one(b0);
            one(edge[0]);
            one(edge[1]);
        }
}

static void check_scalars() {
    const double gams[5] = {0.0, 0x1p-70, 0.5, 0.95, 1.0 - 0x1p-53};
    for (int k = 0; k < 5; k++) {
        int D = 0;                                      // the definition: the smallest D with gam^(2^D) < 2^-64, capped
        double w = gams[k];
        while (D < 64 && !(w < 0x1p-64)) { w = w * w; D++; }
        CHECK(doubling_rounds(gams[k]) == D);
    }
    CHECK(doubling_rounds(0.0) == 0 && doubling_rounds(0x1p-70) == 0 && doubling_rounds(0.5) == 7);
    CHECK(doubling_rounds(1.0 - 0x1p-53) == 59);       // (1 - 2^-53)^(2^59) ~ exp(-64) < 2^-64 <= (1 - 2^-53)^(2^58)
    CHECK(rel_loss(3.0, 3.0) == 0.0);                   // equal values, NaN-free even at 0 / 0
    CHECK(rel_loss(0.0, -1.0) == 0.0);                  // V* = 0: no relative loss is defined
    CHECK(rel_loss(4.0, 3.0) == 0.25 && rel_loss(-4.0, -5.0) == -0.25);
    CHECK(rel_loss(0.0, 0.0) == 0.0);
    CHECK(improve_margin(0.5, 0x1p-10) == 0x1p-10);     // 2 * 0.25 * tol / 0.5
    CHECK(improve_margin(0.0, 1.0) == 0.0);
    CHECK(noise_blend(0.75, 4.0, 0.25, 8.0) == 5.0);
    const double q[4] = {1.0, 3.0, 3.0, 2.0};
    double bv = -1.0;
    CHECK(first_max(4, [&](int k) { return q[k]; }, bv) == 1 && bv == 3.0);      // the first of two equal maxima
    CHECK(first_max(1, [&](int k) { return q[k]; }, bv) == 0 && bv == 1.0);
    // keys order attractors by basin, then by the smaller rep; a key gives its rep back; 0 stands for none
    CHECK(attr_key(2, 5) > attr_key(1, 0) && attr_key(2, 3) > attr_key(2, 5));
    CHECK(attr_key_rep(attr_key(1, 0)) == 0 && attr_key_rep(attr_key(4096, 4095)) == 4095 && attr_key_rep(0) == -1);
    CHECK(attr_key(1, 0xffff) != 0);
}

int main() {
    long maps = 0;
    for (int n = 1; n <= kMaxStates; n++) {
        long count = 1;
        for (int i = 0; i < n; i++) count *= n;
        for (long code = 0; code < count; code++) {
            uint16_t F[kMaxStates];
            long c = code;
            for (int i = 0; i < n; i++) { F[i] = (uint16_t)(c % n); c /= n; }
            maps++;
            check_walk(F, n);
            check_doubling(F, n);
        }
    }
    CHECK(maps == 3413);
    check_band();
    check_scalars();
    if (g_failed) {
        printf("solve dev check: %d failures\n", g_failed);
        return 1;
    }
    printf("solve dev ok: %ld maps\n", maps);
    return 0;
}
