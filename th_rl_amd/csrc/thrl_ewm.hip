// thrl_ewm.hip -- exponentially weighted mean of per-game episode rows, carried across calls (thrl_ewm_rows,
// include/thrl.h): the kernel and, beside it, the entry point with its checks.  A stream: every row is read once and
// written once, and each thread walks its own column in episode order, so the result does not depend on the launch
// geometry or on the cut of the episodes into calls.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "thrl_host.h"

using namespace thrl::host;

namespace thrl {

namespace {

constexpr int kEwmBlock = 256;            // 4 waves
constexpr int kEwmAhead = 4;              // rows whose loads are in flight ahead of the one being smoothed

struct EwmArgs {
    int64_t G;
    int32_t N, E;
    double decay, den;
    const double* rew;
    const double* act;
    double* rew_out;
    double* act_out;
    const double* state_in;
    double* state_out;
};

// One thread per (state row j = blockIdx.y, game g): lanes consecutive in g, so every load and store of a wave is one
// contiguous 512 B.  The loads of the next kEwmAhead rows are issued before the multiply-add-divide of the current
// one (their addresses do not depend on it); in place this is safe too, a thread reads row e + kEwmAhead of its own
// column before it writes row e.
__global__ void __launch_bounds__(kEwmBlock) k_ewm_rows(const EwmArgs a) {
    const int64_t G = a.G;
    const int64_t g = (int64_t)blockIdx.x * kEwmBlock + threadIdx.x;
    if (g >= G) return;
    const int j = (int)blockIdx.y;
    const bool is_rew = j < a.N;
    const int64_t plane = (int64_t)a.N * G;
    const int64_t col = (int64_t)(is_rew ? j : j - a.N) * G + g;
    const double* in = (is_rew ? a.rew : a.act) + col;
    double* out = (is_rew ? a.rew_out : a.act_out) + col;
    const int64_t s = (int64_t)j * G + g;
    const int64_t E = a.E;
    const double d = a.decay;
    double num = a.state_in ? a.state_in[s] : 0.0;
    double den = a.den;
    if (E < 1) return;
    const int64_t last = E - 1;
    // Two register sets of kEwmAhead rows: while one is smoothed the other's loads are in flight.  The loads in the
    // loop are unconditional, with the row clamped to the last one (a value past the end is loaded again and not
    // used): a load under a branch is waited for where the branch joins, not where its value is first used.
    double x[kEwmAhead], y[kEwmAhead];
#pragma unroll
    for (int k = 0; k < kEwmAhead; k++) x[k] = in[(k < last ? (int64_t)k : last) * plane];
    int64_t e = 0;
    for (; e + 2 * kEwmAhead <= E; e += 2 * kEwmAhead) {
#pragma unroll
        for (int k = 0; k < kEwmAhead; k++) y[k] = in[(e + kEwmAhead + k) * plane];
#pragma unroll
        for (int k = 0; k < kEwmAhead; k++) {
            num = x[k] + d * num;                                   // two roundings each (-ffp-contract=off)
            den = 1.0 + d * den;
            out[(e + k) * plane] = num / den;
        }
#pragma unroll
        for (int k = 0; k < kEwmAhead; k++) {
            const int64_t nx = e + 2 * kEwmAhead + k;
            x[k] = in[(nx < last ? nx : last) * plane];
        }
#pragma unroll
        for (int k = 0; k < kEwmAhead; k++) {
            num = y[k] + d * num;
            den = 1.0 + d * den;
            out[(e + kEwmAhead + k) * plane] = num / den;
        }
    }
    // fewer than 2 * kEwmAhead rows are left: x holds the first kEwmAhead of them
#pragma unroll
    for (int k = 0; k < kEwmAhead; k++) {
        if (e + k < E) {
            num = x[k] + d * num;
            den = 1.0 + d * den;
            out[(e + k) * plane] = num / den;
        }
    }
    for (int64_t r = e + kEwmAhead; r < E; r++) {
        num = in[r * plane] + d * num;
        den = 1.0 + d * den;
        out[r * plane] = num / den;
    }
    a.state_out[s] = num;
}

// [p, p + n) and [q, q + m) share a byte
bool overlaps(const void* p, uint64_t n, const void* q, uint64_t m) {
    const uint64_t a = (uint64_t)(uintptr_t)p, b = (uint64_t)(uintptr_t)q;
    return n > 0 && m > 0 && a < b + m && b < a + n;
}

}  // namespace

}  // namespace thrl

extern "C" int thrl_ewm_rows(const thrl_ewm_rows_args* x, void* stream) {
    using namespace thrl;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->n_agents < 1 || x->n_agents > THRL_MAXA)
        return fail(THRL_ERR_BAD_CONFIG, "n_agents=%d out of [1,%d]", x->n_agents, THRL_MAXA);
    if (x->n_episodes < 0) return fail(THRL_ERR_BAD_CONFIG, "n_episodes=%d must be >= 0", x->n_episodes);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved must be 0");
    if (!(x->decay > 0.0 && x->decay < 1.0)) return fail(THRL_ERR_BAD_CONFIG, "decay=%g must lie in (0, 1)", x->decay);
    if (!(x->den >= 0.0) || !isfinite(x->den)) return fail(THRL_ERR_BAD_CONFIG, "den=%g must be finite and >= 0", x->den);
    if (!x->reward_rows || !x->action_rows || !x->reward_out || !x->action_out)
        return fail(THRL_ERR_NULL, "reward_rows / action_rows / reward_out / action_out is NULL");
    const uint64_t rows = (uint64_t)x->n_episodes * (uint64_t)x->n_agents * (uint64_t)x->n_games * sizeof(double);
    const uint64_t st = 2ull * (uint64_t)x->n_agents * (uint64_t)x->n_games * sizeof(double);
    if ((x->reward_out != x->reward_rows && overlaps(x->reward_out, rows, x->reward_rows, rows))
        || (x->action_out != x->action_rows && overlaps(x->action_out, rows, x->action_rows, rows)))
        return fail(THRL_ERR_BAD_CONFIG, "an output overlaps its input without being the input itself (in place)");
    if (overlaps(x->reward_out, rows, x->action_rows, rows) || overlaps(x->action_out, rows, x->reward_rows, rows)
        || overlaps(x->reward_out, rows, x->action_out, rows))
        return fail(THRL_ERR_BAD_CONFIG, "reward_out / action_out overlap each other or the other's input");
    if (!x->state_out) return fail(THRL_ERR_NULL, "state_out is NULL");
    if (x->state_in && x->state_in != x->state_out && overlaps(x->state_out, st, x->state_in, st))
        return fail(THRL_ERR_BAD_CONFIG, "state_out overlaps state_in without being equal to it");
    if (overlaps(x->state_out, st, x->reward_rows, rows) || overlaps(x->state_out, st, x->action_rows, rows)
        || overlaps(x->state_out, st, x->reward_out, rows) || overlaps(x->state_out, st, x->action_out, rows))
        return fail(THRL_ERR_BAD_CONFIG, "state_out overlaps the rows");
    double den = x->den;
    for (int e = 0; e < x->n_episodes; e++) den = 1.0 + x->decay * den;     // the kernel's own sequence
    if (x->n_episodes > 0) {
        EwmArgs a;
        memset(&a, 0, sizeof(a));
        a.G = x->n_games; a.N = x->n_agents; a.E = x->n_episodes;
        a.decay = x->decay; a.den = x->den;
        a.rew = x->reward_rows; a.act = x->action_rows; a.rew_out = x->reward_out; a.act_out = x->action_out;
        a.state_in = x->state_in; a.state_out = x->state_out;
        const unsigned gx = (unsigned)((a.G + kEwmBlock - 1) / kEwmBlock);
        hipLaunchKernelGGL(k_ewm_rows, dim3(gx, (unsigned)(2 * a.N)), dim3(kEwmBlock), 0, (hipStream_t)stream, a);
        const int e = (int)hipGetLastError();
        if (e) return hip_fail(e, "k_ewm_rows launch");
    }
    if (x->den_out) *x->den_out = den;
    return THRL_OK;
}
