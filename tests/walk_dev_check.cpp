// walk_dev_check.cpp -- a stand-alone host program over the cycle search of th_rl_amd/csrc/thrl_walk_dev.h, the one
// k_deviation, k_xplay_walk, k_tp_walk and k_ta_deviation share.  The search is integer code, so it is checked here
// exhaustively against a plain first-repeat search (an array of first-visit steps, nothing of Brent's): every map F on
// n states for n = 1 .. 5 (3,413 maps), every start, every horizon H from 1 to n + 2, both values of want_s.  Once with
// the state as one int, and with the state number spread over N = 2 rows of a tuple of MAXN = 2 and over N = 3 rows of
// a tuple of MAXN = 8, where the map scribbles over the entries past N at every application: they are neither read nor
// compared, or the results would differ.  tests/test_walk_dev_host.py builds it as host code with
// -fsanitize=address,undefined and runs it.  It makes no HIP call.
#include "../th_rl_amd/csrc/thrl_walk_dev.h"

#include <stdio.h>

using namespace thrl;

static int g_failed = 0;
static long g_cases = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { if (g_failed < 20) printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

constexpr int kMaxStates = 5;
constexpr int kJunk = 1000;          // entries past N hold values from here up: no state number reaches them

struct Ref {
    bool found;
    int mu, lam, s;
};

// the first repeat of x0, F(x0), ..: mu the first visit of the repeated state, lam the steps since; found iff mu + lam <= H
static Ref reference(const int* F, int n, int x0, int H) {
    int first[kMaxStates];
    for (int k = 0; k < n; k++) first[k] = -1;
    int x = x0, t = 0;
    while (first[x] < 0) { first[x] = t++; x = F[x]; }
    Ref r;
    r.mu = first[x];
    r.lam = t - first[x];
    r.found = r.mu + r.lam <= H;
    r.s = x0;
    if (r.found) {
        for (int j = 0; j < r.mu; j++) r.s = F[r.s];
    } else {
        r.mu = H;
        r.lam = 0;
        for (int j = 0; j < H; j++) r.s = F[r.s];
    }
    return r;
}

// state number k over N rows, every row needed to tell two states apart
template <int N>
static void to_rows(int k, int* x) {
    if (N == 2) { x[0] = k / 3; x[1] = k % 3; }
    else { x[0] = k & 1; x[1] = (k >> 1) & 1; x[2] = k >> 2; }
}

template <int N>
static int from_rows(const int* x) {
    return N == 2 ? x[0] * 3 + x[1] : x[0] + 2 * x[1] + 4 * x[2];
}

static void check_scalar(const int* F, int n, int x0, int H, bool want_s, const Ref& r) {
    const int untouched = -7;
    int mu = -1, lam = -1, s = untouched;
    const bool found = find_cycle(x0, 1, H, [&](int& x) { x = F[x]; }, mu, lam, s, want_s);
    CHECK(found == r.found && mu == r.mu && lam == r.lam);
    CHECK(s == (r.found || want_s ? r.s : untouched));
    (void)n;
}

template <int MAXN, int N>
static void check_rows(const int* F, int x0, int H, bool want_s, const Ref& r) {
    int junk = kJunk;
    const auto scribble = [&](int* x) { for (int i = N; i < MAXN; i++) x[i] = junk++; };
    int start[MAXN], s[MAXN], s_before[MAXN];
    to_rows<N>(x0, start);
    scribble(start);
    for (int i = 0; i < MAXN; i++) s[i] = s_before[i] = -7 - i;
    int mu = -1, lam = -1;
    const bool found = find_cycle(start, N, H, [&](int* x) {
        int k = from_rows<N>(x);
        CHECK(k >= 0 && k < kMaxStates);
        if (k < 0 || k >= kMaxStates) k = 0;
        to_rows<N>(F[k], x);
        scribble(x);
    }, mu, lam, s, want_s);
    CHECK(found == r.found && mu == r.mu && lam == r.lam);
    if (r.found || want_s) CHECK(from_rows<N>(s) == r.s);
    else for (int i = 0; i < N; i++) CHECK(s[i] == s_before[i]);
    // the search writes nothing past N (where it walks s to x_H, the map itself scribbles there)
    if (r.found || !want_s)
        for (int i = N; i < MAXN; i++) CHECK(s[i] == s_before[i]);
}

int main() {
    long maps = 0;
    for (int n = 1; n <= kMaxStates; n++) {
        long count = 1;
        for (int i = 0; i < n; i++) count *= n;
        for (long code = 0; code < count; code++) {
            int F[kMaxStates];
            long c = code;
            for (int i = 0; i < n; i++) { F[i] = (int)(c % n); c /= n; }
            maps++;
            for (int x0 = 0; x0 < n; x0++)
                for (int H = 1; H <= n + 2; H++) {
                    const Ref r = reference(F, n, x0, H);
                    for (int w = 0; w < 2; w++) {
                        check_scalar(F, n, x0, H, w != 0, r);
                        check_rows<2, 2>(F, x0, H, w != 0, r);
                        check_rows<8, 3>(F, x0, H, w != 0, r);
                        g_cases++;
                    }
                }
        }
    }
    CHECK(maps == 3413);
    // copy_rows / same_rows on their own: entries past N are left alone and not compared
    {
        int x[8] = {1, 2, 3, 40, 50, 60, 70, 80}, y[8] = {1, 2, 3, 41, 51, 61, 71, 81}, d[8] = {0, 0, 0, 9, 9, 9, 9, 9};
        CHECK(same_rows<8>(x, y, 3) && !same_rows<8>(x, y, 4));
        copy_rows<8>(d, x, 3);
        CHECK(d[0] == 1 && d[1] == 2 && d[2] == 3 && d[3] == 9 && d[7] == 9);
    }
    if (g_failed) {
        printf("walk dev check: %d failures\n", g_failed);
        return 1;
    }
    printf("walk dev ok: %ld maps, %ld cases per state shape\n", maps, g_cases);
    return 0;
}
