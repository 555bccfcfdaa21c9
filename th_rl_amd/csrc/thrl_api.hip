// thrl_api.hip -- the extern "C" surface of libthrl_hip.so (see include/thrl.h).
// Host logic only: validation, kernel selection, launch geometry.  No torch types.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "thrl_attractors.h"
#include "thrl_stationary.h"
#include "thrl_converge.h"
#include "thrl_crossplay.h"
#include "thrl_deviation.h"
#include "thrl_equilibrium.h"
#include "thrl_kernels.h"
#include "thrl_tuple_analysis.h"
#include "thrl_tuple_attractors.h"
#include "thrl_tuple_play.h"
#include "thrl_sampled.h"
#include "thrl_sampled_noise.h"
#include "thrl_tuple_stationary.h"
#include "thrl_wave_lut.h"

using namespace thrl;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(int e, const char* what) {
    return fail(THRL_ERR_HIP, "%s: %s", what, hipGetErrorString((hipError_t)e));
}

// ---- host restatements of the tiny scalar formulas (IEEE double/float; this
// file is built with -ffp-contract=off so they round exactly like the device).
double h_scale(int k, const thrl_cfg* c, int i) {
    double x = (double)k / ((double)c->n_actions[i] - 1.0);
    x = x * (c->act_hi[i] - c->act_lo[i]);
    return x + c->act_lo[i];
}
int h_encode64(double price, const thrl_cfg* c, int i) {
    return (int)rint(price / c->max_state[i] * (double)c->n_states[i]);
}
int h_encode32(double price, const thrl_cfg* c, int i) {
    float x = (float)price;
    x = x / (float)c->max_state[i];
    x = x * (float)c->n_states[i];
    return (int)rintf(x);
}
int validate(const thrl_cfg* c) {
    if (!c) return fail(THRL_ERR_NULL, "cfg is NULL");
    if (c->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", c->n_games);
    if (c->n_agents < 1 || c->n_agents > THRL_MAXA)
        return fail(THRL_ERR_BAD_CONFIG, "n_agents=%d out of [1,%d]", c->n_agents, THRL_MAXA);
    if (c->max_steps < 1) return fail(THRL_ERR_BAD_CONFIG, "max_steps=%d must be >= 1", c->max_steps);
    if (c->q_dtype != 0 && c->q_dtype != 1) return fail(THRL_ERR_BAD_CONFIG, "q_dtype=%d", c->q_dtype);
    if (!(c->env_b != 0.0)) return fail(THRL_ERR_BAD_CONFIG, "env_b must be non-zero");
    for (int i = 0; i < c->n_agents; i++) {
        if (c->n_states[i] < 1 || c->n_states[i] > 32000)
            return fail(THRL_ERR_BAD_CONFIG, "agent %d: states=%d out of [1,32000]", i, c->n_states[i]);
        if (c->n_actions[i] < 2 || c->n_actions[i] > 32000)
            return fail(THRL_ERR_BAD_CONFIG, "agent %d: actions=%d out of [2,32000]", i, c->n_actions[i]);
        if (c->capacity[i] < 0 || c->min_memory[i] < 0)
            return fail(THRL_ERR_BAD_CONFIG, "agent %d: negative capacity/min_memory", i);
        if (!(c->max_state[i] > 0.0)) return fail(THRL_ERR_BAD_CONFIG, "agent %d: max_state must be > 0", i);
    }
    return THRL_OK;
}

void fill_agents(const thrl_cfg* c, AgentParams* ag, EnvParams* env) {
    int off = 0;
    for (int i = 0; i < THRL_MAXA; i++) {
        AgentParams p;
        memset(&p, 0, sizeof(p));
        if (i < c->n_agents) {
            p.rows = c->n_states[i] + 1;
            p.n_states = c->n_states[i];
            p.n_actions = c->n_actions[i];
            p.min_memory = c->min_memory[i];
            p.capacity = c->capacity[i];
            p.table_off = off;
            off += p.rows * p.n_actions;
            p.max_state = c->max_state[i];
            p.max_state_f = (float)c->max_state[i];
            p.inv_max_state = 1.0 / c->max_state[i];
            p.inv_max_state_f = 1.0f / p.max_state_f;
            p.gamma = c->gamma[i]; p.alpha = c->alpha[i];
            p.one_minus_alpha = 1.0 - c->alpha[i];
            p.gamma_f = (float)c->gamma[i]; p.alpha_f = (float)c->alpha[i];
            p.one_minus_alpha_f = (float)(1.0 - c->alpha[i]);
            p.alpha_gamma_f = p.alpha_f * p.gamma_f;
            p.eps_end = c->eps_end[i]; p.eps_step = c->eps_step[i];
            p.act_lo = c->act_lo[i]; p.act_span = c->act_hi[i] - c->act_lo[i];
            p.act_den = (double)c->n_actions[i] - 1.0;
        }
        ag[i] = p;
    }
    if (env) {
        env->a = c->env_a; env->b = c->env_b; env->ratio = c->env_a / c->env_b;
        env->noise_prob = c->noise_prob; env->noise_lo = c->env_a * 0.7;
    }
}

// Rows reachable after a transition, per agent [lo, hi]: the price is monotone in every agent's action index (scale,
// the products, the sum, b * Q and a - b * Q are monotone roundings, the clamp at 0 too), and so is encode64, so the
// extremes of every agent's next row lie at the 2^N corners of the action grid.
void reach_window(const thrl_cfg* c, int* lo, int* hi) {
    const int N = c->n_agents;
    for (int i = 0; i < N; i++) { lo[i] = c->n_states[i]; hi[i] = 0; }
    const double ratio = c->env_a / c->env_b;
    for (int mask = 0; mask < (1 << N); mask++) {
        double Q = 0.0;
        for (int j = 0; j < N; j++) {
            const double A = ratio * h_scale((mask >> j) & 1 ? c->n_actions[j] - 1 : 0, c, j);
            Q = Q + A;
        }
        double p = c->env_a - c->env_b * Q;
        if (!(p > 0.0)) p = 0.0;
        for (int i = 0; i < N; i++) {
            int r = h_encode64(p, c, i);
            r = r < 0 ? 0 : (r > c->n_states[i] ? c->n_states[i] : r);
            if (r < lo[i]) lo[i] = r;
            if (r > hi[i]) hi[i] = r;
        }
    }
}

// largest number of buffered transitions any agent can hold (bounds the ring)
int eff_capacity(const thrl_cfg* c, int i) {
    const int cap = c->capacity[i], mm = c->min_memory[i], T = c->max_steps;
    if (cap <= 0) return 0;
    if (cap < mm) return cap;                        // never trains, ring wraps at cap
    const long need = (long)T * ((mm + T - 1) / T > 0 ? (mm + T - 1) / T : 1);
    return (int)(need < cap ? need : cap);
}
int capmax_of(const thrl_cfg* c) {
    int m = 1;
    for (int i = 0; i < c->n_agents; i++) { int e = eff_capacity(c, i); if (e > m) m = e; }
    return m;
}

struct WavePlan {
    bool ok;
    char why[200];
    int row_lo, win_rows;
    int epk, replay_from;           // training cycle: episodes per train_net that trains, first kept transition
    int lut_bytes, game_lds_bytes, waves_per_block, blocks_per_cu;
    // closed-form play tables (thrl_wave_kernel.h play_affine): both encodes of every action pair's price are the local row
    // aff_c - aff_m0 * a0 - aff_m1 * a1, and the configuration is one the plain float32 kernel with one row register plays
    int affine, aff_c, aff_m0, aff_m1;
};

// Per-device figures the launch geometry needs.  A read-only cache keyed by the HIP device id (filled
// once per device under a mutex; the only process-wide state besides the thread-local error string).
// Without a visible device (the CPU-side tests of the host logic) the MI355X figures are assumed.
struct DevInfo { int cus, lds_per_cu, waves_per_cu; };
constexpr DevInfo kMi355x = {256, 160 * 1024, 32};
constexpr int kMaxDevices = 64;

DevInfo dev_info() {
    static std::mutex mu;
    static DevInfo cache[kMaxDevices];
    static bool have[kMaxDevices] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        return kMi355x;
    }
    std::lock_guard<std::mutex> lock(mu);
    if (!have[dev]) {
        DevInfo d = kMi355x;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return kMi355x; }
        if (prop.multiProcessorCount > 0) d.cus = prop.multiProcessorCount;       // 256; 32 per XCD partition
        if (prop.maxSharedMemoryPerMultiProcessor >= 64 * 1024) d.lds_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
        if (prop.maxThreadsPerMultiProcessor >= 64) d.waves_per_cu = prop.maxThreadsPerMultiProcessor / 64;
        cache[dev] = d;
        have[dev] = true;
    }
    return cache[dev];
}

// THRL_WAVE_MAX_WAVES_PER_CU: tuning / diagnostic knob, read ONCE per process (not per call)
int env_wave_cap() {
    static std::once_flag once;
    static int cap = 0;
    std::call_once(once, [] {
        if (const char* e = getenv("THRL_WAVE_MAX_WAVES_PER_CU")) { const int v = atoi(e); if (v >= 1 && v <= 64) cap = v; }
    });
    return cap;
}

// THRL_WAVE_AFFINE=0: diagnostic switch, keeps affine payoff grids on the payoff-LUT path (A/B runs inside one build);
// read ONCE per process
bool env_wave_affine() {
    static std::once_flag once;
    static bool on = true;
    std::call_once(once, [] { if (const char* e = getenv("THRL_WAVE_AFFINE")) on = atoi(e) != 0; });
    return on;
}

// Can the fused wave kernel run this config?  (DESIGN.md "wave kernel: eligibility")
WavePlan plan_wave(const thrl_cfg* c, const thrl_run* run, bool injected) {
    WavePlan p;
    memset(&p, 0, sizeof(p));
#define NO(msg) do { snprintf(p.why, sizeof(p.why), "%s", msg); return p; } while (0)
    if (c->n_agents != 2) NO("needs exactly 2 agents");
    if (c->n_states[0] != c->n_states[1] || c->n_actions[0] != c->n_actions[1] ||
        c->max_state[0] != c->max_state[1]) NO("agents must share the state/action grid sizes");
    const int A = c->n_actions[0], T = c->max_steps;
    if (A > 32) NO("actions > 32");
    // Training cycle (buffers.py:12-19, agents.py:60,77): after every episode len(memory) = min(appends,
    // capacity); train_net trains -- and empties the buffer -- once that reaches min_memory, i.e. every
    // epk = ceil(min_memory / T)-th episode, on the last min(epk*T, capacity) transitions.  Both agents
    // must share the cycle and the kept suffix (or both never train: capacity < min_memory).
    int epk = 0, keep = 0;
    for (int i = 0; i < 2; i++) {
        const int cap = c->capacity[i], mm = c->min_memory[i] > 0 ? c->min_memory[i] : 1;
        const int k_i = cap >= mm && cap > 0 ? (mm + T - 1) / T : 0;           // 0: never trains
        const int keep_i = k_i ? (k_i * T < cap ? k_i * T : cap) : 0;
        if (i == 0) { epk = k_i; keep = keep_i; }
        else if (k_i != epk || keep_i != keep) NO("the agents' replay buffers fill / train on different cycles");
        if (run && run->mem_count[i] != 0) NO("non-empty replay memory on entry");
    }
    const bool never = epk == 0;
    if (never) epk = 1;
    if ((long)epk * T > 256) NO("more than 256 transitions per training cycle");
    if (epk > kWaveMaxEpisodes) NO("more than 32 episodes per training cycle");
    if (run && run->n_episodes % epk != 0) NO("episodes of this call are not a multiple of the training cycle");
    p.epk = epk;
    p.replay_from = never ? epk * T : epk * T - keep;
    // Row window = every row a step can land in: both encodes (play: float32, train: float64)
    // of the price on the whole action grid; with noise the intercept ranges over [0.7a, a).
    int lo = 1 << 30, hi = -1;
    const double ratio = c->env_a / c->env_b;
    // is the row affine in the action indices, row = rc - rm0 * a0 - rm1 * a1, under both encodes?  (noise-free price only;
    // the slopes come from the pairs (1, 0) and (0, 1), every pair is then tested against them)
    bool affine = !(c->noise_prob > 0.0);
    int rc = 0, rm0 = 0, rm1 = 0;
    for (int a0 = 0; a0 < A; a0++)
        for (int a1 = 0; a1 < A; a1++) {
            double Q = 0.0;
            Q = Q + ratio * h_scale(a0, c, 0);
            Q = Q + ratio * h_scale(a1, c, 1);
            const double intercepts[2] = {c->env_a, c->env_a * 0.7};
            for (int z = 0; z < (c->noise_prob > 0.0 ? 2 : 1); z++) {
                double price = intercepts[z] - c->env_b * Q;
                if (!(price > 0.0)) price = 0.0;
                const int r64 = h_encode64(price, c, 0), r32 = h_encode32(price, c, 0);
                if (r64 < 0 || r64 > c->n_states[0] || r32 < 0 || r32 > c->n_states[0])
                    NO("price outside the table on the action grid");
                if (r64 < lo) lo = r64;
                if (r32 < lo) lo = r32;
                if (r64 > hi) hi = r64;
                if (r32 > hi) hi = r32;
                if (z == 0 && affine) {                              // (a1 is the inner loop: (0,0), (0,1) ... come first)
                    if (a0 == 0 && a1 == 0) rc = r32;
                    else if (a0 == 0 && a1 == 1) rm1 = rc - r32;
                    else if (a0 == 1 && a1 == 0) rm0 = rc - r32;
                    if (r32 != r64 || r32 != rc - rm0 * a0 - rm1 * a1) affine = false;
                }
            }
        }
    p.row_lo = lo;
    p.win_rows = hi - lo + 1;
    if (p.win_rows + 2 > 128) NO("reachable row window > 126 rows");
    const WaveLut L = wave_lut_layout(A);
    p.lut_bytes = L.lds_bytes;          // LDS-staged part of the LUT image
    p.game_lds_bytes = 2 * (p.win_rows + 2) * A * (c->q_dtype == 1 ? 8 : 4);
    if (c->q_dtype == 0 && !(c->noise_prob > 0.0)) p.game_lds_bytes += 256;       // per-step words of half a segment (thrl_wave_kernel.h kLdsMK)
    // Closed-form play tables where the kLdsMK path would run outside training cycles: float32 tables, no noise, one row
    // register, one episode per cycle with nothing dropped.  (Sweeps and the GREEDY variant are decided per call: launch_wave.)
    // Non-negative slopes and rc - lo < 62 make every byte of the packed arithmetic stay inside its byte.
    if (affine && rm0 >= 0 && rm1 >= 0 && c->q_dtype == 0 && p.win_rows + 2 <= 64 && p.epk == 1 && p.replay_from == 0 &&
        rc - lo >= 0 && rc - lo < p.win_rows && rc - rm0 * (A - 1) - rm1 * (A - 1) >= lo && env_wave_affine()) {
        p.affine = 1; p.aff_c = rc - lo; p.aff_m0 = rm0; p.aff_m1 = rm1;
    }
    // choose waves/block to maximise resident waves per CU (LDS-bound); a block may take the whole CU's LDS
    int best_w = 0, best_total = 0, best_b = 0;
    const DevInfo dv = dev_info();
    int cap_waves = dv.waves_per_cu;
    if (env_wave_cap() > 0 && env_wave_cap() < cap_waves) cap_waves = env_wave_cap();
    // Most resident waves wins (throughput is latency-bound and scales with them).  A block's waves
    // are dealt to the CU's 4 SIMDs in turn, so among equal totals blocks of 4k waves are preferred
    // (they load the SIMDs evenly); with games handed out dynamically an uneven split only costs the
    // crowded SIMD's waves some speed (noise window: 3 x 5 waves measured 12 % faster than 3 x 4).
    // register limit: the float32 variants are compiled for 5 waves/SIMD (4 with noise or T > 128),
    // the float64 ones (twice the LDS per game) for 3
    const int reg_waves = 4 * (c->q_dtype == 1 ? 3 : ((c->noise_prob > 0.0 || c->max_steps * p.epk > 128) ? 4 : 5));
    if (cap_waves > reg_waves) cap_waves = reg_waves;
    for (int w = 1; w <= 16; w++) {
        const int lds = p.lut_bytes + w * p.game_lds_bytes;
        if (lds > dv.lds_per_cu) break;
        int b = dv.lds_per_cu / (((lds + 511) / 512) * 512);
        if (b * w > cap_waves) b = cap_waves / w;
        if (b < 1) continue;
        const int total = b * w;
        const bool even = (w & 3) == 0, best_even = best_w > 0 && (best_w & 3) == 0;
        if (total > best_total || (total == best_total && ((even && !best_even) || (even == best_even && w < best_w)))) {
            best_total = total; best_w = w; best_b = b;
        }
    }
    if (best_w == 0) NO("table window does not fit LDS");
    p.waves_per_block = best_w;
    p.blocks_per_cu = best_b;
    p.ok = true;
    return p;
#undef NO
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- the tuple-chain kernel (thrl_tuple_kernel.h): 1-4 QTable agents with individual grids, state = action tuple
struct TuplePlan {
    bool ok;
    char why[200];
    TupleArgs a;                    // geometry fields filled: tuples, windows, LDS layout, LUT offsets
    int waves_per_block, blocks_per_cu;
    size_t lut_image_bytes;
};
constexpr size_t kTupleWsBytes = 160 * 1024;       // LUT image (< 128 KiB) + the launch's work counter in the last 64 bytes;
                                                   // the visit log of the resident waves follows (tuple_workspace)

TuplePlan plan_tuple(const thrl_cfg* c, const thrl_run* run) {
    TuplePlan p;
    memset(&p, 0, sizeof(p));
#define NO(msg) do { snprintf(p.why, sizeof(p.why), "%s", msg); return p; } while (0)
    const int N = c->n_agents, T = c->max_steps;
    if (N < 1 || N > kTupMaxN) NO("more than 4 agents");
    if (T > 256) NO("more than 256 steps per episode");
    long tuples = 1;
    for (int i = 0; i < N; i++) {
        if (c->n_actions[i] > 64) NO("more than 64 actions");
        tuples *= c->n_actions[i];
        if (tuples > kTupMaxTuples) NO("more than 4,096 action tuples");
        // train_net must train -- and empty the buffer -- after every episode, on exactly that episode's transitions
        // (buffers.py:12-19, agents.py:60,77): min_memory <= T <= capacity
        if (!(c->min_memory[i] <= T && T <= c->capacity[i])) NO("replay buffer does not fill / train once per episode");
        if (run && run->mem_count[i] != 0) NO("non-empty replay memory on entry");
    }
    TupleArgs& a = p.a;
    a.N = N; a.T = T; a.tuples = (int)tuples;
    // row windows: both encodes of the price of every tuple; with noise the intercept ranges over [0.7a, a]
    // (environments.py:29-31) and both encodes are monotonic in the price, so the two ends cover the range
    int lo[kTupMaxN], hi[kTupMaxN];
    for (int i = 0; i < N; i++) { lo[i] = 1 << 30; hi[i] = -1; }
    const double ratio = c->env_a / c->env_b;
    int digit[kTupMaxN] = {0, 0, 0, 0};
    for (long t = 0; t < tuples; t++) {
        double Q = 0.0;
        for (int i = 0; i < N; i++) Q = Q + ratio * h_scale(digit[i], c, i);
        const double intercepts[2] = {c->env_a, c->env_a * 0.7};
        for (int v = 0; v < (c->noise_prob > 0.0 ? 2 : 1); v++) {
            double price = intercepts[v] - c->env_b * Q;
            if (!(price > 0.0)) price = 0.0;
            for (int i = 0; i < N; i++) {
                const int r64 = h_encode64(price, c, i), r32 = h_encode32(price, c, i);
                if (r64 < 0 || r64 > c->n_states[i] || r32 < 0 || r32 > c->n_states[i]) NO("price outside a table on the action grid");
                lo[i] = r64 < lo[i] ? r64 : lo[i]; lo[i] = r32 < lo[i] ? r32 : lo[i];
                hi[i] = r64 > hi[i] ? r64 : hi[i]; hi[i] = r32 > hi[i] ? r32 : hi[i];
            }
        }
        for (int i = N - 1; i >= 0; i--) { if (++digit[i] < c->n_actions[i]) break; digit[i] = 0; }     // last agent = fastest digit
    }
    const int esz = c->q_dtype == 1 ? 8 : 4;
    int elems = 0, am = 0, hd = 0;
    for (int i = 0; i < N; i++) {
        a.row_lo[i] = lo[i]; a.win_rows[i] = hi[i] - lo[i] + 1;
        if (a.win_rows[i] + 2 > 256) NO("reachable row window > 254 rows");
        const int cells = (a.win_rows[i] + 2) * c->n_actions[i];
        if (cells > 65535) NO("more than 65,535 resident table cells per agent");
        a.tab_off[i] = elems; elems += (cells + 3) & ~3;
        a.am_off_i[i] = am; am += (a.win_rows[i] + 2 + 3) & ~3;
        a.hist_off_i[i] = hd; hd += (cells + 1) / 2;
    }
    a.am_off = (int)align_up((size_t)elems * esz, 16);
    a.g_off = (int)align_up((size_t)a.am_off + am, 16);
    a.hist_dwords = hd;
    if ((size_t)hd * 4 > (size_t)elems * esz) NO("visit histogram does not fit the table region");      // (never: u16 per cell)
    a.game_lds_bytes = (int)align_up((size_t)a.g_off + 2 * ((size_t)tuples + 1), 16);
    // action words: agent i's action in a bit field of ceil(log2 A_i) bits; the widths sum to < log2(tuples) + N <= 16
    // (the fields start at bit 1 and the LAST agent's comes first: its field, masked, is its action x 2 = the byte offset of
    // its term in a u16 table indexed by the tuple -- the play chain of thrl_tuple_kernel.h adds it without a multiply)
    int sh = 1;
    for (int i = N - 1; i >= 0; i--) {
        int bits = 0;
        while ((1 << bits) < c->n_actions[i]) bits++;
        a.act_sh[i] = sh; a.act_bits[i] = bits; sh += bits;
    }
    if (sh > 16) NO("action word wider than 16 bits");
    a.vlog_wave_bytes = (int64_t)kTupMaxEpisodes * T * (N <= 2 ? 4 : 8);
    a.aq_off = (int)align_up((size_t)tuples * 8, 16);           // prow [tuples] u32, trow [tuples] u32
    a.lut_lds_bytes = a.aq_off + N * 64 * 8 * 2;
    a.price_off = a.lut_lds_bytes;
    a.qsum_off = a.price_off + 8 * (int)tuples;
    p.lut_image_bytes = (size_t)a.qsum_off + 8 * (size_t)tuples;
    if (p.lut_image_bytes > kTupleWsBytes - 64) NO("LUT image too large");
    const DevInfo dv = dev_info();
    int cap_waves = dv.waves_per_cu < 16 ? dv.waves_per_cu : 16;         // the kernel is compiled for 4 waves per SIMD
    int best_w = 0, best_total = 0, best_b = 0;
    for (int w = 1; w <= 16; w++) {
        const int lds = a.lut_lds_bytes + w * a.game_lds_bytes;
        if (lds > dv.lds_per_cu) break;
        int b = dv.lds_per_cu / (((lds + 511) / 512) * 512);
        if (b * w > cap_waves) b = cap_waves / w;
        if (b < 1) continue;
        const int total = b * w;
        const bool even = (w & 3) == 0, best_even = best_w > 0 && (best_w & 3) == 0;
        if (total > best_total || (total == best_total && ((even && !best_even) || (even == best_even && w < best_w)))) {
            best_total = total; best_w = w; best_b = b;
        }
    }
    if (best_w == 0) NO("tables of one game do not fit LDS");
    p.waves_per_block = best_w; p.blocks_per_cu = best_b;
    p.ok = true;
    return p;
#undef NO
}

// Workspace of the tuple-chain kernel: [0, kTupleWsBytes) LUT image + work counter, then the visit log of every resident wave
struct TupleWs { int grid, total_waves; size_t bytes; };
TupleWs tuple_workspace(const thrl_cfg* c, const TuplePlan& p) {
    TupleWs w;
    w.grid = (c->n_games + p.waves_per_block - 1) / p.waves_per_block;
    const int max_grid = dev_info().cus * p.blocks_per_cu;
    if (w.grid > max_grid) w.grid = max_grid;
    w.total_waves = w.grid * p.waves_per_block;
    w.bytes = kTupleWsBytes + align_up((size_t)w.total_waves * (size_t)p.a.vlog_wave_bytes, 256);
    return w;
}

constexpr size_t kLutRegion = 16384;            // workspace bytes reserved for the LUT image

// Workspace of the wave kernel, sized from the config and the current device:
//   [0, kLutRegion)   payoff-LUT image (+ the launch's work counter in its last 64 bytes)
//   partial           [total_waves][kWaveMaxEpisodes][4] fixed-point log sums
//   tlog              [total_waves][kWaveMaxEpisodes][NSEG][64] cell words of the transitions (visit counters)
// total_waves = the persistent grid: resident blocks per CU x CUs, or fewer when G is small.
struct WaveWs { int grid, total_waves; size_t partial_off, tlog_off, bytes; };
WaveWs wave_workspace(const thrl_cfg* c, const WavePlan& p) {
    WaveWs w;
    w.grid = (c->n_games + p.waves_per_block - 1) / p.waves_per_block;
    const int max_grid = dev_info().cus * p.blocks_per_cu;
    if (w.grid > max_grid) w.grid = max_grid;
    w.total_waves = w.grid * p.waves_per_block;
    const size_t nseg = (size_t)(c->max_steps * p.epk + 63) / 64;
    w.partial_off = kLutRegion;
    w.tlog_off = w.partial_off + align_up((size_t)w.total_waves * 4 * kWaveMaxEpisodes * sizeof(long long), 256);
    w.bytes = w.tlog_off + align_up((size_t)w.total_waves * kWaveMaxEpisodes * nseg * 64 * sizeof(uint32_t), 256);
    return w;
}

}  // namespace

namespace thrl { int launch_group_stats(const thrl_group_stats_args* g, hipStream_t s); }   // thrl_stats.hip

// power of two (a double with mantissa exactly 0.5 after frexp), positive and finite
static bool pow2(double x) {
    int ex;
    return x > 0.0 && isfinite(x) && frexp(x, &ex) == 0.5;
}

extern "C" {

int thrl_version(void) { return THRL_ABI_VERSION; }
const char* thrl_last_error(void) { return g_err; }

// th_rl_amd/build.py passes the ablation mask of the build and a hash of the sources
#ifndef THRL_BUILD_ABLATE
#define THRL_BUILD_ABLATE 0
#endif
#ifndef THRL_SRC_HASH
#define THRL_SRC_HASH "unknown"
#endif
#ifndef THRL_WAVE_HASH
#define THRL_WAVE_HASH "unknown"
#endif
#ifndef THRL_NN_HASH
#define THRL_NN_HASH "unknown"
#endif
#define THRL_STR2(x) #x
#define THRL_STR(x) THRL_STR2(x)
const char* thrl_build_info(void) {
    return "abi=" THRL_STR(THRL_ABI_VERSION) ";ablate=" THRL_STR(THRL_BUILD_ABLATE) ";src=" THRL_SRC_HASH
           ";wave=" THRL_WAVE_HASH ";nn=" THRL_NN_HASH;
}
int thrl_ablate_mask(void) { return THRL_BUILD_ABLATE; }

size_t thrl_table_stride(const thrl_cfg* c) {
    if (!c || c->n_agents < 1 || c->n_agents > THRL_MAXA) return 0;
    size_t s = 0;
    for (int i = 0; i < c->n_agents; i++) s += (size_t)(c->n_states[i] + 1) * (size_t)c->n_actions[i];
    return s;
}
size_t thrl_table_offset(const thrl_cfg* c, int agent) {
    if (!c || agent < 0 || agent > c->n_agents) return 0;
    size_t s = 0;
    for (int i = 0; i < agent; i++) s += (size_t)(c->n_states[i] + 1) * (size_t)c->n_actions[i];
    return s;
}
size_t thrl_replay_mem_bytes(const thrl_cfg* c) {
    if (validate(c) != THRL_OK) return 0;
    const size_t n = (size_t)capmax_of(c) * (size_t)c->n_agents * (size_t)c->n_games;
    return align_up(n * 2, 256) * 3 + align_up(n * 8, 256) * 2;
}
size_t thrl_workspace_bytes(const thrl_cfg* c) {
    if (validate(c) != THRL_OK) return 0;
    const WavePlan p = plan_wave(c, nullptr, false);
    const TuplePlan tp = plan_tuple(c, nullptr);
    const size_t tuple_ws = tp.ok ? tuple_workspace(c, tp).bytes : kLutRegion;       // (the generic kernel keeps nothing there)
    if (!p.ok) return tuple_ws;
    const size_t wave_ws = wave_workspace(c, p).bytes;                               // (either kernel can be asked for by id)
    return wave_ws > tuple_ws ? wave_ws : tuple_ws;
}
int thrl_select_kernel(const thrl_cfg* c, int injected) {
    if (validate(c) != THRL_OK) return THRL_ERR_BAD_CONFIG;
    const WavePlan p = plan_wave(c, nullptr, injected != 0);
    if (!p.ok) {
        const TuplePlan tp = plan_tuple(c, nullptr);
        if (tp.ok) return THRL_KERNEL_TUPLE;
        snprintf(g_err, sizeof(g_err), "generic kernel: %s; %s", p.why, tp.why);
        return THRL_KERNEL_GENERIC;
    }
    return THRL_KERNEL_WAVE;
}

int thrl_wave_play_form(const thrl_cfg* c, int out_c_m0_m1[3]) {
    if (validate(c) != THRL_OK) return 0;
    const WavePlan p = plan_wave(c, nullptr, false);
    if (!p.ok || !p.affine) return 0;
    if (out_c_m0_m1) { out_c_m0_m1[0] = p.aff_c; out_c_m0_m1[1] = p.aff_m0; out_c_m0_m1[2] = p.aff_m1; }
    return 1;
}

int thrl_training_cycle(const thrl_cfg* c) {
    if (validate(c) != THRL_OK) return 0;
    const WavePlan p = plan_wave(c, nullptr, false);
    return p.ok ? p.epk : 0;
}

int thrl_qtable_init(const thrl_cfg* c, void* q, int32_t* counter, double* state, uint64_t seed,
                     uint64_t game_offset, const double* sweep_gamma, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!q || !state) return fail(THRL_ERR_NULL, "q/state is NULL");
    InitArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.N = c->n_agents; a.stride = (int64_t)thrl_table_stride(c); a.env_a = c->env_a;
    fill_agents(c, a.ag, nullptr);
    a.q = q; a.counter = counter; a.state = state; a.seed = seed; a.game_offset = game_offset;
    a.sw_gamma = sweep_gamma;
    const int e = launch_init(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_init launch") : THRL_OK;
}

static int run_generic(const thrl_cfg* c, const thrl_buffers* b, thrl_run* run, hipStream_t s) {
    if ((b->sweep_eps_end || b->sweep_eps_step) && !b->sweep_eps)
        return fail(THRL_ERR_NULL, "sweep_eps_end / sweep_eps_step need the per-game epsilon state sweep_eps");
    if (b->sweep_noise_prob && !(c->noise_prob > 0.0))
        return fail(THRL_ERR_BAD_CONFIG, "sweep_noise_prob needs cfg.noise_prob > 0 (it switches the noise draws on)");
    const int capmax = capmax_of(c);
    const size_t need = thrl_replay_mem_bytes(c);
    if (!b->replay_mem || b->replay_mem_bytes < need)
        return fail(THRL_ERR_WORKSPACE, "replay_mem too small: have %zu need %zu", b->replay_mem_bytes, need);
    const bool injected = b->inj_u != nullptr;
    if (injected && !b->inj_choice) return fail(THRL_ERR_NULL, "inj_u given without inj_choice");
    if (injected && c->noise_prob > 0.0 && (!b->inj_noise_u || !b->inj_noise_a))
        return fail(THRL_ERR_NULL, "noise_prob > 0 with injected draws needs inj_noise_u/inj_noise_a");
    GenericArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.N = c->n_agents; a.T = c->max_steps; a.capmax = capmax;
    a.stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a.ag, &a.env);
    a.q = b->q; a.counter = b->counter; a.state = b->state;
    {
        const size_t n = (size_t)capmax * (size_t)c->n_agents * (size_t)c->n_games;
        char* base = (char*)b->replay_mem;
        const size_t s2 = align_up(n * 2, 256), s8 = align_up(n * 8, 256);
        a.mem.s = (int16_t*)base; a.mem.ns = (int16_t*)(base + s2); a.mem.a = (int16_t*)(base + 2 * s2);
        a.mem.r = (double*)(base + 3 * s2); a.mem.ov = (double*)(base + 3 * s2 + s8);
    }
    a.sum_reward = b->reward_log; a.sum_action = b->action_log;
    if ((a.sum_reward == nullptr) != (a.sum_action == nullptr))
        return fail(THRL_ERR_NULL, "reward_log and action_log must both be given or both NULL");
    a.game_reward_log = b->game_reward_log; a.game_action_log = b->game_action_log;
    a.inj_u = b->inj_u; a.inj_choice = b->inj_choice; a.inj_noise_u = b->inj_noise_u; a.inj_noise_a = b->inj_noise_a;
    a.seed = run->seed; a.game_offset = run->game_offset; a.first_episode = run->first_episode;
    a.n_episodes = run->n_episodes;
    for (int i = 0; i < THRL_MAXA; i++) { a.eps0[i] = run->eps[i]; a.cnt0[i] = run->mem_count[i]; }
    a.sw_gamma = b->sweep_gamma; a.sw_alpha = b->sweep_alpha; a.sw_eps_end = b->sweep_eps_end;
    a.sw_eps_step = b->sweep_eps_step; a.sw_eps = b->sweep_eps; a.sw_noise_prob = b->sweep_noise_prob;
    const int nlog = run->n_episodes * c->n_agents;
    if (a.sum_reward) {
        hipError_t e1 = hipMemsetAsync(a.sum_reward, 0, sizeof(double) * nlog, s);
        hipError_t e2 = hipMemsetAsync(a.sum_action, 0, sizeof(double) * nlog, s);
        if (e1 != hipSuccess || e2 != hipSuccess) return hip_fail(e1 != hipSuccess ? e1 : e2, "log memset");
    }
    int e = launch_generic(a, c->q_dtype, s);
    if (e) return hip_fail(e, "k_generic_episodes launch");
    if (a.sum_reward) {
        e = launch_finalize_logs(a.sum_reward, a.sum_action, nlog, c->n_games, s);
        if (e) return hip_fail(e, "k_finalize_logs launch");
    }
    // host mirror of the per-episode bookkeeping that is identical for all games
    for (int ep = 0; ep < run->n_episodes; ep++)
        for (int i = 0; i < c->n_agents; i++) {
            const int cap = c->capacity[i];
            if (cap > 0)
                for (int t = 0; t < c->max_steps; t++) {
                    run->mem_count[i] += 1;
                    if (run->mem_count[i] >= 2 * cap) run->mem_count[i] -= cap;
                }
            const int len = run->mem_count[i] < cap ? run->mem_count[i] : cap;
            if (len >= c->min_memory[i]) run->mem_count[i] = 0;
            run->eps[i] = c->eps_end[i] + (run->eps[i] - c->eps_end[i]) * c->eps_step[i];
        }
    run->kernel_used = THRL_KERNEL_GENERIC;
    return THRL_OK;
}

static int run_wave(const thrl_cfg* c, const thrl_buffers* b, thrl_run* run, const WavePlan& p, int force_variant, hipStream_t s) {
    if (b->inj_u && !b->inj_choice) return fail(THRL_ERR_NULL, "inj_u given without inj_choice");
    if (b->inj_u && c->noise_prob > 0.0 && (!b->inj_noise_u || !b->inj_noise_a))
        return fail(THRL_ERR_NULL, "noise_prob > 0 with injected draws needs inj_noise_u/inj_noise_a");
    if (!b->workspace || b->workspace_bytes < thrl_workspace_bytes(c))
        return fail(THRL_ERR_WORKSPACE, "workspace too small: have %zu need %zu", b->workspace_bytes,
                    thrl_workspace_bytes(c));
    if (wave_lut_layout(c->n_actions[0]).bytes > (int)kLutRegion - 64) return fail(THRL_ERR_UNSUPPORTED, "LUT image too large");
    WaveArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.T = c->max_steps; a.A = c->n_actions[0]; a.rows = c->n_states[0] + 1;
    a.row_lo = p.row_lo; a.win_rows = p.win_rows;
    a.epk = p.epk; a.replay_from = p.replay_from;
    a.aff_on = p.affine; a.aff_c = p.aff_c; a.aff_m0 = p.aff_m0; a.aff_m1 = p.aff_m1;
    a.waves_per_block = p.waves_per_block;
    a.force_variant = force_variant;
    a.lut_bytes = p.lut_bytes; a.game_lds_bytes = p.game_lds_bytes;
    a.stride = (int64_t)thrl_table_stride(c);
    AgentParams ag[THRL_MAXA];
    fill_agents(c, ag, &a.env);
    a.ag[0] = ag[0]; a.ag[1] = ag[1];
    a.q = b->q; a.counter = b->counter; a.state = b->state;
    unsigned char* lut = (unsigned char*)b->workspace;
    a.lut_ns = lut;
    const WaveWs ws = wave_workspace(c, p);
    a.partial = (long long*)((char*)b->workspace + ws.partial_off);
    {   // fixed-point scales of the log sums: 2^s with G * (bound of one game's episode mean) * 2^s <= 2^62
        double hi = 0.0;
        for (int i = 0; i < 2; i++) hi = fmax(hi, fmax(fabs(c->act_lo[i]), fabs(c->act_hi[i])));
        const double bound[2] = {fmax(c->env_a * (c->env_a / c->env_b) * hi, 1e-300), fmax(hi, 1e-300)};
        for (int k = 0; k < 2; k++) {
            int ex = 0;
            frexp((double)c->n_games * bound[k], &ex);          // G*bound < 2^ex
            int sh = 62 - ex;
            sh = sh > 60 ? 60 : (sh < 0 ? 0 : sh);
            a.log_scale[k] = ldexp(1.0, sh);
        }
    }
    a.tlog = (uint32_t*)((char*)b->workspace + ws.tlog_off);
    const size_t game_rows = (size_t)2 * (size_t)c->n_games;        // per-game log elements per episode
    a.next_game = (int32_t*)((char*)b->workspace + kLutRegion - 64);       // the LUT image is < 16 KiB - 64
    a.seed = run->seed; a.game_offset = run->game_offset;
    a.sw_gamma = b->sweep_gamma; a.sw_alpha = b->sweep_alpha; a.sw_eps_end = b->sweep_eps_end;
    a.sw_eps_step = b->sweep_eps_step; a.sw_eps = b->sweep_eps; a.sw_noise_prob = b->sweep_noise_prob;
    if ((b->sweep_eps_end || b->sweep_eps_step) && !b->sweep_eps)
        return fail(THRL_ERR_NULL, "sweep_eps_end / sweep_eps_step need the per-game epsilon state sweep_eps");
    if (b->sweep_noise_prob && !(c->noise_prob > 0.0))
        return fail(THRL_ERR_BAD_CONFIG, "sweep_noise_prob needs cfg.noise_prob > 0 (it sizes the row window)");
    const int chunk_max = kWaveMaxEpisodes / p.epk * p.epk;        // whole training cycles per launch
    if (force_variant == 2 && (p.epk > 1 || p.replay_from > 0 || c->noise_prob > 0.0 || b->sweep_gamma || b->sweep_alpha ||
                               b->sweep_eps_end || b->sweep_eps_step || b->sweep_eps || b->sweep_noise_prob))
        return fail(THRL_ERR_UNSUPPORTED, "THRL_KERNEL_WAVE_GREEDY: no greedy-regime variant for noise, sweeps or "
                                          "multi-episode training cycles");

    const int block = p.waves_per_block * 64;
    const int grid = ws.grid;                             // persistent grid; games are handed out by a work counter
    a.total_waves = ws.total_waves;
    const size_t lds = (size_t)p.lut_bytes + (size_t)p.waves_per_block * p.game_lds_bytes;

    int e = launch_wave_lut(a, lut, s);
    if (e) return hip_fail(e, "k_wave_lut launch");
    int done = 0;
    while (done < run->n_episodes) {
        const int n = run->n_episodes - done < chunk_max ? run->n_episodes - done : chunk_max;
        a.n_episodes = n;
        a.first_episode = run->first_episode + (uint64_t)done;
        a.game_reward_log = b->game_reward_log ? b->game_reward_log + (size_t)done * game_rows : nullptr;
        a.game_action_log = b->game_action_log ? b->game_action_log + (size_t)done * game_rows : nullptr;
        if (b->inj_u) {                                  // parity mode: this chunk's slice of the draws
            const size_t per_ep = (size_t)c->max_steps * 2 * (size_t)c->n_games;
            a.inj_u = b->inj_u + (size_t)done * per_ep;
            a.inj_choice = b->inj_choice + (size_t)done * per_ep;
            if (c->noise_prob > 0.0) {
                a.inj_noise_u = b->inj_noise_u + (size_t)done * (per_ep / 2);
                a.inj_noise_a = b->inj_noise_a + (size_t)done * (per_ep / 2);
            }
        }
        for (int ep = 0; ep < n; ep++)
            for (int i = 0; i < 2; i++) {
                a.eps[ep][i] = run->eps[i];
                run->eps[i] = c->eps_end[i] + (run->eps[i] - c->eps_end[i]) * c->eps_step[i];
            }
        if (hipMemsetAsync(a.next_game, 0, sizeof(int32_t), s) != hipSuccess) return hip_fail((int)hipGetLastError(), "hipMemsetAsync");
        e = launch_wave(a, c->q_dtype, grid, block, lds, s);
        if (e) return hip_fail(e, "k_wave_episodes launch");
        if (b->reward_log || b->action_log) {
            e = launch_wave_reduce(a.partial, a.log_scale, a.total_waves, n, c->n_games,
                                   b->reward_log ? b->reward_log + (size_t)done * 2 : nullptr,
                                   b->action_log ? b->action_log + (size_t)done * 2 : nullptr, s);
            if (e) return hip_fail(e, "k_wave_reduce launch");
        }
        done += n;
    }
    run->kernel_used = THRL_KERNEL_WAVE;
    return THRL_OK;
}

static int run_tuple(const thrl_cfg* c, const thrl_buffers* b, thrl_run* run, TuplePlan& p, hipStream_t s) {
    if (b->inj_u && !b->inj_choice) return fail(THRL_ERR_NULL, "inj_u given without inj_choice");
    if (b->sweep_noise_prob && !(c->noise_prob > 0.0))
        return fail(THRL_ERR_BAD_CONFIG, "sweep_noise_prob needs cfg.noise_prob > 0 (it switches the noise draws on)");
    if (b->inj_u && c->noise_prob > 0.0 && (!b->inj_noise_u || !b->inj_noise_a))
        return fail(THRL_ERR_NULL, "injected draws with noise_prob > 0 need inj_noise_u / inj_noise_a");
    const TupleWs ws = tuple_workspace(c, p);
    if (!b->workspace || b->workspace_bytes < ws.bytes)
        return fail(THRL_ERR_WORKSPACE, "workspace too small: have %zu need %zu", b->workspace_bytes, ws.bytes);
    if ((b->reward_log == nullptr) != (b->action_log == nullptr))
        return fail(THRL_ERR_NULL, "reward_log and action_log must both be given or both NULL");
    TupleArgs& a = p.a;
    a.G = c->n_games;
    a.stride = (int64_t)thrl_table_stride(c);
    AgentParams ag[THRL_MAXA];
    fill_agents(c, ag, &a.env);
    for (int i = 0; i < a.N; i++) a.ag[i] = ag[i];
    a.q = b->q; a.counter = b->counter; a.state = b->state;
    a.sw_gamma = b->sweep_gamma; a.sw_alpha = b->sweep_alpha; a.sw_eps_end = b->sweep_eps_end;
    a.sw_eps_step = b->sweep_eps_step; a.sw_eps = b->sweep_eps; a.sw_noise_prob = b->sweep_noise_prob;
    unsigned char* lut = (unsigned char*)b->workspace;
    a.lut = lut;
    a.next_game = (int32_t*)((char*)b->workspace + kTupleWsBytes - 64);
    a.vlog = (char*)b->workspace + kTupleWsBytes;
    a.seed = run->seed; a.game_offset = run->game_offset;
    a.waves_per_block = p.waves_per_block;
    const int grid = ws.grid;
    a.total_waves = ws.total_waves;
    const int block = p.waves_per_block * 64;
    const size_t lds = (size_t)a.lut_lds_bytes + (size_t)p.waves_per_block * a.game_lds_bytes;
    int e = launch_tuple_lut(a, lut, s);
    if (e) return hip_fail(e, "k_tuple_lut launch");
    const int nlog = run->n_episodes * c->n_agents;
    if (b->reward_log) {
        hipError_t e1 = hipMemsetAsync(b->reward_log, 0, sizeof(double) * nlog, s);
        hipError_t e2 = hipMemsetAsync(b->action_log, 0, sizeof(double) * nlog, s);
        if (e1 != hipSuccess || e2 != hipSuccess) return hip_fail(e1 != hipSuccess ? e1 : e2, "log memset");
    }
    int done = 0;
    while (done < run->n_episodes) {
        const int n = run->n_episodes - done < kTupMaxEpisodes ? run->n_episodes - done : kTupMaxEpisodes;
        a.n_episodes = n;
        a.first_episode = run->first_episode + (uint64_t)done;
        a.sum_reward = b->reward_log ? b->reward_log + (size_t)done * a.N : nullptr;
        a.sum_action = b->action_log ? b->action_log + (size_t)done * a.N : nullptr;
        a.game_reward_log = b->game_reward_log ? b->game_reward_log + (size_t)done * a.N * (size_t)c->n_games : nullptr;
        a.game_action_log = b->game_action_log ? b->game_action_log + (size_t)done * a.N * (size_t)c->n_games : nullptr;
        if (b->inj_u) {
            const size_t per_ep = (size_t)c->max_steps * a.N * (size_t)c->n_games;
            a.inj_u = b->inj_u + (size_t)done * per_ep;
            a.inj_choice = b->inj_choice + (size_t)done * per_ep;
            if (c->noise_prob > 0.0) {
                a.inj_noise_u = b->inj_noise_u + (size_t)done * c->max_steps * (size_t)c->n_games;
                a.inj_noise_a = b->inj_noise_a + (size_t)done * c->max_steps * (size_t)c->n_games;
            }
        }
        for (int ep = 0; ep < n; ep++)
            for (int i = 0; i < a.N; i++) {
                a.eps[ep][i] = run->eps[i];
                run->eps[i] = c->eps_end[i] + (run->eps[i] - c->eps_end[i]) * c->eps_step[i];       // agents.py:78
            }
        if (hipMemsetAsync(a.next_game, 0, sizeof(int32_t), s) != hipSuccess) return hip_fail((int)hipGetLastError(), "hipMemsetAsync");
        e = launch_tuple(a, c->q_dtype, grid, block, lds, s);
        if (e) return hip_fail(e, "k_tuple_episodes launch");
        done += n;
    }
    if (b->reward_log) {
        e = launch_finalize_logs(b->reward_log, b->action_log, nlog, c->n_games, s);
        if (e) return hip_fail(e, "k_finalize_logs launch");
    }
    run->kernel_used = THRL_KERNEL_TUPLE;
    return THRL_OK;
}

int thrl_qtable_episodes(const thrl_cfg* c, const thrl_buffers* b, thrl_run* run, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!b || !run) return fail(THRL_ERR_NULL, "bufs/run is NULL");
    if (!b->q || !b->state) return fail(THRL_ERR_NULL, "q/state is NULL");
    if (run->n_episodes < 0) return fail(THRL_ERR_BAD_CONFIG, "n_episodes < 0");
    run->kernel_used = 0;
    if (run->n_episodes == 0) return THRL_OK;
    const bool injected = b->inj_u != nullptr;
    int k = run->kernel;
    if (k != THRL_KERNEL_AUTO && k != THRL_KERNEL_GENERIC && k != THRL_KERNEL_WAVE && k != THRL_KERNEL_WAVE_PLAIN &&
        k != THRL_KERNEL_WAVE_GREEDY && k != THRL_KERNEL_TUPLE)
        return fail(THRL_ERR_BAD_CONFIG, "unknown kernel id %d", k);
    const bool any_sweep = b->sweep_gamma || b->sweep_alpha || b->sweep_eps_end || b->sweep_eps_step || b->sweep_eps || b->sweep_noise_prob;
    if (k == THRL_KERNEL_TUPLE || k == THRL_KERNEL_AUTO) {
        // (AUTO prefers the two-agent wave kernel where it applies: decided below; the tuple kernel takes what that one cannot)
        TuplePlan tp = plan_tuple(c, run);
        if (tp.ok && (b->sweep_eps_end || b->sweep_eps_step) && !b->sweep_eps) {
            // a game's epsilon must survive from launch to launch: it lives in sweep_eps
            tp.ok = false; snprintf(tp.why, sizeof(tp.why), "epsilon-schedule sweep without a per-game epsilon array (sweep_eps)");
        }
        tp.a.sweep = any_sweep ? 1 : 0;
        if (k == THRL_KERNEL_TUPLE) {
            if (!tp.ok) return fail(THRL_ERR_UNSUPPORTED, "tuple kernel cannot run this config: %s", tp.why);
            return run_tuple(c, b, run, tp, (hipStream_t)stream);
        }
        if (tp.ok && !plan_wave(c, run, injected).ok) return run_tuple(c, b, run, tp, (hipStream_t)stream);
    }
    const int force_variant = k == THRL_KERNEL_WAVE_PLAIN ? 1 : (k == THRL_KERNEL_WAVE_GREEDY ? 2 : 0);
    if (force_variant) k = THRL_KERNEL_WAVE;
    if (k != THRL_KERNEL_GENERIC) {
        WavePlan p = plan_wave(c, run, injected);
        if (p.ok && (p.epk > 1 || p.replay_from > 0) && (b->sweep_gamma || b->sweep_alpha || b->sweep_eps_end || b->sweep_eps_step || b->sweep_eps || b->sweep_noise_prob)) {
            p.ok = false; snprintf(p.why, sizeof(p.why), "per-game sweeps with a multi-episode training cycle or a truncated deque");
        }
        if (p.ok) return run_wave(c, b, run, p, force_variant, (hipStream_t)stream);
        if (k == THRL_KERNEL_WAVE) return fail(THRL_ERR_UNSUPPORTED, "wave kernel cannot run this config: %s", p.why);
    }
    return run_generic(c, b, run, (hipStream_t)stream);
}

int thrl_play_greedy(const thrl_cfg* c, const void* q, const double* state0, int32_t iters, uint64_t seed,
                     uint64_t game_offset, double* mean_reward, double* mean_action, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!q || !mean_reward || !mean_action) return fail(THRL_ERR_NULL, "q/mean_reward/mean_action is NULL");
    if (iters < 0) return fail(THRL_ERR_BAD_CONFIG, "iters < 0");
    if (iters == 0) return THRL_OK;
    PlayArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.N = c->n_agents; a.T = c->max_steps; a.iters = iters;
    a.stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a.ag, &a.env);
    a.q = q; a.state0 = state0; a.mean_reward = mean_reward; a.mean_action = mean_action;
    a.seed = seed; a.game_offset = game_offset;
    const int e = launch_play(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_play_greedy launch") : THRL_OK;
}

static int op_common(const thrl_cfg* c, OpArgs* a) {
    int rc = validate(c);
    if (rc) return rc;
    memset(a, 0, sizeof(*a));
    a->G = c->n_games; a->N = c->n_agents; a->stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a->ag, &a->env);
    return THRL_OK;
}

int thrl_op_sample_action(const thrl_cfg* c, int agent, const void* q, const double* price, double eps,
                          const double* u, const int8_t* choice, int encode32, int32_t* action_out,
                          void* stream) {
    OpArgs a;
    int rc = op_common(c, &a);
    if (rc) return rc;
    if (agent < 0 || agent >= c->n_agents) return fail(THRL_ERR_BAD_CONFIG, "agent %d out of range", agent);
    if (!q || !price || !action_out) return fail(THRL_ERR_NULL, "q/price/action_out is NULL");
    if (u && !choice) return fail(THRL_ERR_NULL, "u given without choice");
    a.agent = agent; a.q = const_cast<void*>(q); a.price = price; a.eps = eps; a.u = u; a.choice = choice;
    a.encode32 = encode32; a.action_out = action_out;
    const int e = launch_op_sample(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_sample launch") : THRL_OK;
}

int thrl_op_encode(const thrl_cfg* c, int agent, const double* price, int as_float32, int32_t* row_out,
                   void* stream) {
    OpArgs a;
    int rc = op_common(c, &a);
    if (rc) return rc;
    if (agent < 0 || agent >= c->n_agents) return fail(THRL_ERR_BAD_CONFIG, "agent %d out of range", agent);
    if (!price || !row_out) return fail(THRL_ERR_NULL, "price/row_out is NULL");
    a.agent = agent; a.price = price; a.encode32 = as_float32; a.action_out = row_out;
    const int e = launch_op_encode(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_encode launch") : THRL_OK;
}

int thrl_op_scale(const thrl_cfg* c, int agent, const int32_t* action, double* scaled_out, void* stream) {
    OpArgs a;
    int rc = op_common(c, &a);
    if (rc) return rc;
    if (agent < 0 || agent >= c->n_agents) return fail(THRL_ERR_BAD_CONFIG, "agent %d out of range", agent);
    if (!action || !scaled_out) return fail(THRL_ERR_NULL, "action/scaled_out is NULL");
    a.agent = agent; a.action = action; a.scaled_out = scaled_out;
    const int e = launch_op_scale(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_scale launch") : THRL_OK;
}

int thrl_op_env_step(const thrl_cfg* c, const double* scaled, const double* noise_u, const double* noise_a,
                     double* price_out, double* reward_out, void* stream) {
    OpArgs a;
    int rc = op_common(c, &a);
    if (rc) return rc;
    if (!scaled || !price_out || !reward_out) return fail(THRL_ERR_NULL, "scaled/price_out/reward_out is NULL");
    if (noise_u && !noise_a) return fail(THRL_ERR_NULL, "noise_u given without noise_a");
    a.scaled = scaled; a.noise_u = noise_u; a.noise_a = noise_a; a.price_out = price_out;
    a.reward_out = reward_out;
    const int e = launch_op_env_step(a, (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_env_step launch") : THRL_OK;
}

int thrl_op_td_update(const thrl_cfg* c, int agent, void* q, int32_t* counter, int32_t n, const double* price,
                      const int32_t* action, const double* reward, const double* next_price, double* scratch,
                      void* stream) {
    OpArgs a;
    int rc = op_common(c, &a);
    if (rc) return rc;
    if (agent < 0 || agent >= c->n_agents) return fail(THRL_ERR_BAD_CONFIG, "agent %d out of range", agent);
    if (n < 0) return fail(THRL_ERR_BAD_CONFIG, "n < 0");
    if (n == 0) return THRL_OK;
    if (!q || !price || !action || !reward || !next_price || !scratch)
        return fail(THRL_ERR_NULL, "a required pointer is NULL");
    a.agent = agent; a.q = q; a.counter = counter; a.n = n; a.price = price; a.action = action;
    a.reward = reward; a.next_price = next_price; a.reward_out = scratch;
    const int e = launch_op_td(a, c->q_dtype, (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_td launch") : THRL_OK;
}

size_t thrl_nn_param_count(int n_actions) {
    if (n_actions < 2 || n_actions > 32) return 0;
    return (size_t)(2 * THRL_NN_HIDDEN + n_actions * THRL_NN_HIDDEN + n_actions);
}

static int nn_check(int n_games, int n_actions) {
    if (n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", n_games);
    if (n_actions < 2 || n_actions > 32) return fail(THRL_ERR_BAD_CONFIG, "neural agent: actions=%d out of [2,32]", n_actions);
    return THRL_OK;
}

int thrl_nn_init(int n_games, int n_actions, float* params, uint64_t seed, uint64_t game_offset, int agent,
                 void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params) return fail(THRL_ERR_NULL, "params is NULL");
    const int e = launch_nn_init(n_games, n_actions, params, seed, game_offset, agent, 0, (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_init launch") : THRL_OK;
}

size_t thrl_ac_param_count(int n_actions) {
    const size_t p = thrl_nn_param_count(n_actions);
    return p ? p + THRL_NN_HIDDEN + 1 : 0;
}

int thrl_ac_init(int n_games, int n_actions, float* params, uint64_t seed, uint64_t game_offset, int agent,
                 void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params) return fail(THRL_ERR_NULL, "params is NULL");
    const int e = launch_nn_init(n_games, n_actions, params, seed, game_offset, agent, 1, (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_init launch") : THRL_OK;
}

int thrl_ac_act(int n_games, int n_actions, const float* params, const double* price, const double* u,
                int32_t* action_out, float* prob_out, void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params || !price || !action_out) return fail(THRL_ERR_NULL, "params/price/action_out is NULL");
    const int e = launch_nn_act(n_games, n_actions, params, (int)thrl_ac_param_count(n_actions), price, u, action_out,
                                prob_out, (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_act launch") : THRL_OK;
}

int thrl_ac_train(int n_games, int n_actions, float* params, float* adam_m, float* adam_v, int32_t step, int32_t n,
                  int32_t ld, const double* price, const int32_t* action, const double* reward, const double* next_price,
                  double gamma, double entropy_coef, double lr, const double* sweep_gamma, const double* sweep_entropy,
                  float* grad_out, void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params || !adam_m || !adam_v || !price || !action || !reward || !next_price)
        return fail(THRL_ERR_NULL, "a required pointer is NULL");
    if (n < 2 || n > THRL_NN_MAX_TRANSITIONS)
        return fail(THRL_ERR_UNSUPPORTED, "n=%d transitions out of [2,%d]", n, THRL_NN_MAX_TRANSITIONS);
    if (step < 0) return fail(THRL_ERR_BAD_CONFIG, "step < 0");
    if (nn_train_lds_bytes(n_actions, n, 1) > 160 * 1024) return fail(THRL_ERR_UNSUPPORTED, "transition buffer does not fit LDS");
    if (ld < n) return fail(THRL_ERR_BAD_CONFIG, "ld=%d < n=%d", ld, n);
    const int e = launch_nn_train(n_games, n_actions, params, adam_m, adam_v, step, n, ld, price, action, reward, next_price,
                                  (float)gamma, (float)entropy_coef, (float)lr, sweep_gamma, sweep_entropy, grad_out, nullptr,
                                  (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_reinforce_train<AC> launch") : THRL_OK;
}

int thrl_nn_act(int n_games, int n_actions, const float* params, const double* price, const double* u,
                int32_t* action_out, float* prob_out, void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params || !price || !action_out) return fail(THRL_ERR_NULL, "params/price/action_out is NULL");
    const int e = launch_nn_act(n_games, n_actions, params, (int)thrl_nn_param_count(n_actions), price, u, action_out,
                                prob_out, (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_act launch") : THRL_OK;
}

int thrl_nn_reinforce_train(int n_games, int n_actions, float* params, float* adam_m, float* adam_v, int32_t step,
                            int32_t n, int32_t ld, const double* price, const int32_t* action, const double* reward,
                            double gamma, double entropy_coef, double lr, const double* sweep_gamma,
                            const double* sweep_entropy, float* grad_out, float* returns_scratch, void* stream) {
    int rc = nn_check(n_games, n_actions);
    if (rc) return rc;
    if (!params || !adam_m || !adam_v || !price || !action || !reward) return fail(THRL_ERR_NULL, "a required pointer is NULL");
    if (n < 2 || n > THRL_NN_MAX_TRANSITIONS)
        return fail(THRL_ERR_UNSUPPORTED, "n=%d transitions out of [2,%d]", n, THRL_NN_MAX_TRANSITIONS);
    if (step < 0) return fail(THRL_ERR_BAD_CONFIG, "step < 0");
    if (nn_train_lds_bytes(n_actions, n, 0) > 160 * 1024) return fail(THRL_ERR_UNSUPPORTED, "transition buffer does not fit LDS");
    if (ld < n) return fail(THRL_ERR_BAD_CONFIG, "ld=%d < n=%d", ld, n);
    const int e = launch_nn_train(n_games, n_actions, params, adam_m, adam_v, step, n, ld, price, action, reward, nullptr,
                                  (float)gamma, (float)entropy_coef, (float)lr, sweep_gamma, sweep_entropy, grad_out, returns_scratch,
                                  (hipStream_t)stream);
    return e ? hip_fail(e, "k_nn_reinforce_train launch") : THRL_OK;
}

// ---- the tuple-chain kernel for two-agent games with discrete neural policies (thrl_ptuple.hip)
struct PTuplePlan { bool ok; char why[160]; PTupleArgs a; int waves_per_block, blocks_per_cu; size_t scratch_bytes; };
constexpr size_t kPTupleLutRegion = 64 * 1024;     // head of thrl_mixed.policy_tab: LUT image + the launch's work counter (last 64 bytes)

static double h_scale_kind(int k, const thrl_cfg* c, int i, int kind) {
    if (kind == 0) return h_scale(k, c, i);
    double x = (double)k / (double)c->n_actions[i];             // Reinforce.scale (agents.py:153-157): action / actions
    x = x * (c->act_hi[i] - c->act_lo[i]);
    return x + c->act_lo[i];
}

static PTuplePlan plan_ptuple(const thrl_cfg* c, const thrl_mixed* mx) {
    PTuplePlan p;
    memset(&p, 0, sizeof(p));
#define NO(msg) do { snprintf(p.why, sizeof(p.why), "%s", msg); return p; } while (0)
    PTupleArgs& a = p.a;
    if (c->n_agents != 2) NO("not a two-agent game");
    const int T = c->max_steps;
    if (T > 256) NO("more than 256 steps per episode");
    a.qi = -1; a.n_r = 0;
    for (int i = 0; i < 2; i++) {
        a.kind[i] = mx->kind[i];
        if (mx->kind[i] == 0) {
            if (a.qi >= 0) NO("no neural agent");
            a.qi = i;
            if (c->n_actions[i] > 64) NO("QTable agent with more than 64 actions");
            // train_net trains -- and empties the ring -- after every episode (agents.py:60,77)
            if (!(mx->buf_len[i] > 0 && mx->min_memory[i] <= T && T <= mx->buf_len[i] && mx->count[i] == 0)) NO("QTable replay buffer does not train once per episode");
        } else if (mx->kind[i] == 1 || mx->kind[i] == 2) {
            if (c->n_actions[i] > 32) NO("neural agent with more than 32 actions");
            if (mx->buf_len[i] < T) NO("a neural agent's replay ring is shorter than an episode");
            a.ri[a.n_r++] = i;
        } else NO("continuous agent");
    }
    if (a.n_r == 0) NO("no neural agent");
    // per-game sweeps: the QTable agent's rows and noise_prob need the kernel's sweep variant (rows of neural agents only reach
    // their update kernels); a game's epsilon must survive the launch in sweep_eps
    const bool q_sweep = mx->sweep_gamma || mx->sweep_alpha || mx->sweep_eps_end || mx->sweep_eps_step || mx->sweep_eps;
    if (a.qi < 0 && mx->sweep_noise_prob) NO("noise_prob sweep without a QTable agent in the game");
    if (a.qi >= 0 && (mx->sweep_eps_end || mx->sweep_eps_step) && !mx->sweep_eps) NO("epsilon-schedule sweep without a per-game epsilon array (sweep_eps)");
    a.sweep = (a.qi >= 0 && (q_sweep || mx->sweep_noise_prob)) ? 1 : 0;
    const long tuples = (long)c->n_actions[0] * c->n_actions[1];
    if (tuples > kTupMaxTuples) NO("more than 4,096 action pairs");
    a.tuples = (int)tuples; a.T = T;
    // distinct float32 prices, in order of first occurrence (the device repeats this enumeration: k_ptuple_lut), and the
    // QTable agent's row window
    static thread_local float seen[kTupMaxTuples];
    int npid = 0, lo = 1 << 30, hi = -1;
    const double ratio = c->env_a / c->env_b;
    for (int a0 = 0; a0 < c->n_actions[0]; a0++)
        for (int a1 = 0; a1 < c->n_actions[1]; a1++) {
            double Q = 0.0;
            Q = Q + ratio * h_scale_kind(a0, c, 0, mx->kind[0]);
            Q = Q + ratio * h_scale_kind(a1, c, 1, mx->kind[1]);
            double price = c->env_a - c->env_b * Q;
            if (!(price > 0.0)) price = 0.0;
            const float x = (float)price;
            int j = 0;
            while (j < npid && memcmp(&seen[j], &x, 4) != 0) j++;
            if (j == npid) seen[npid++] = x;
            if (a.qi >= 0) {
                // (with env noise the intercept ranges over [0.7a, a]: both encodes are monotonic in the price)
                const double intercepts[2] = {c->env_a, c->env_a * 0.7};
                for (int v = 0; v < (c->noise_prob > 0.0 ? 2 : 1); v++) {
                    double pr = intercepts[v] - c->env_b * Q;
                    if (!(pr > 0.0)) pr = 0.0;
                    const int r64 = h_encode64(pr, c, a.qi), r32 = h_encode32(pr, c, a.qi);
                    if (r64 < 0 || r64 > c->n_states[a.qi] || r32 < 0 || r32 > c->n_states[a.qi]) NO("price outside the table on the action grid");
                    lo = r64 < lo ? r64 : lo; lo = r32 < lo ? r32 : lo;
                    hi = r64 > hi ? r64 : hi; hi = r32 > hi ? r32 : hi;
                }
            }
        }
    if (npid > 2048) NO("more than 2,048 distinct prices");
    a.npid = npid;
    int amax = 0;
    for (int r = 0; r < a.n_r; r++) amax = c->n_actions[a.ri[r]] > amax ? c->n_actions[a.ri[r]] : amax;
    const int apad = amax <= 24 ? 24 : 32;
    const int esz = c->q_dtype == 1 ? 8 : 4;
    size_t off = 0;
    if (a.qi >= 0) {
        a.row_lo = lo; a.win_rows = hi - lo + 1;
        if (a.win_rows + 2 > 256) NO("reachable row window > 254 rows");
        const int cells = (a.win_rows + 2) * c->n_actions[a.qi];
        off = align_up((size_t)cells * esz, 16);
        a.am_off = (int)off; off = align_up(off + a.win_rows + 2, 16);
        a.g_off = (int)off; off = align_up(off + (size_t)tuples + 1, 16);
        a.hist_off = (int)off; a.hist_dwords = (cells + 1) / 2; off = align_up(off + 4 * (size_t)a.hist_dwords, 16);
    }
    a.cdf_off = (int)off;
    if (a.n_r == 2) {
        const size_t cdf = (size_t)2 * (npid + 1) * apad * 4;
        if (cdf > 24 * 1024) NO("price grid too large for in-LDS policy tables");
        off = align_up(off + cdf, 16);
    }
    a.logs_off = (int)off; off += 64 * 4 * 8;
    a.game_lds_bytes = (int)align_up(off, 16);
    a.qrows_off = (int)align_up((size_t)tuples * 2, 16);
    a.xf_off = (int)align_up((size_t)a.qrows_off + (size_t)tuples * 2, 16);
    a.aq_off = (int)align_up((size_t)a.xf_off + (size_t)npid * 4, 16);
    a.lut_lds_bytes = a.aq_off + 2 * 128 * 8;
    a.price_off = a.lut_lds_bytes;
    a.qsum_off = a.price_off + 8 * (int)tuples;
    if ((size_t)a.qsum_off + 8 * (size_t)tuples > kPTupleLutRegion - 64) NO("LUT image too large");
    p.scratch_bytes = kPTupleLutRegion + (a.n_r == 1 ? (size_t)c->n_games * (size_t)(npid + 1) * apad * 4 : 0);
    const DevInfo dv = dev_info();
    const int cap_waves = a.n_r == 1 ? 12 : 16;                     // compiled for 3 / 4 waves per SIMD
    int best_w = 0, best_total = 0, best_b = 0;
    for (int w = 1; w <= 8; w++) {
        const int lds = a.lut_lds_bytes + w * a.game_lds_bytes;
        if (lds > dv.lds_per_cu) break;
        int b = dv.lds_per_cu / (((lds + 511) / 512) * 512);
        if (b * w > cap_waves) b = cap_waves / w;
        if (b < 1) continue;
        const int total = b * w;
        const bool even = (w & 3) == 0, best_even = best_w > 0 && (best_w & 3) == 0;
        if (total > best_total || (total == best_total && ((even && !best_even) || (even == best_even && w < best_w)))) {
            best_total = total; best_w = w; best_b = b;
        }
    }
    if (best_w == 0) NO("one game does not fit LDS");
    p.waves_per_block = best_w; p.blocks_per_cu = best_b;
    p.ok = true;
    return p;
#undef NO
}

int thrl_mixed_episodes(const thrl_cfg* c, thrl_mixed* mx, void* q, int32_t* counter, double* state, thrl_run* run,
                        double* game_reward_log, double* game_action_log, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!mx || !q || !state || !run || !game_reward_log || !game_action_log)
        return fail(THRL_ERR_NULL, "a required pointer is NULL");
    if (run->n_episodes < 0) return fail(THRL_ERR_BAD_CONFIG, "n_episodes < 0");
    if (run->n_episodes == 0) return THRL_OK;
    run->kernel_used = 0;                          // THRL_KERNEL_TUPLE when the tuple-chain kernel ran
    MixedArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.N = c->n_agents; a.T = c->max_steps; a.n_episodes = run->n_episodes;
    a.stride = (int64_t)thrl_table_stride(c);
    fill_agents(c, a.ag, &a.env);
    a.q = q; a.counter = counter; a.state = state;
    a.game_reward_log = game_reward_log; a.game_action_log = game_action_log;
    a.seed = run->seed; a.game_offset = run->game_offset; a.first_episode = run->first_episode;
    for (int i = 0; i < c->n_agents; i++) {
        if (mx->kind[i] < 0 || mx->kind[i] > 3) return fail(THRL_ERR_BAD_CONFIG, "agent %d: unknown kind %d", i, mx->kind[i]);
        if (mx->kind[i] != 0 && (!mx->nn_params[i] || (mx->kind[i] != 3 && c->n_actions[i] > 32)))
            return fail(THRL_ERR_NULL, "agent %d: a neural agent needs nn_params and actions <= 32", i);
        a.nn_stride[i] = mx->kind[i] == 2 ? (int32_t)thrl_ac_param_count(c->n_actions[i])
                                          : (int32_t)thrl_nn_param_count(c->n_actions[i]);
        if (mx->buf_len[i] > 0 && (!mx->buf_price[i] || !mx->buf_action[i] || !mx->buf_reward[i] || !mx->buf_nprice[i]))
            return fail(THRL_ERR_NULL, "agent %d: replay buffer pointers are NULL", i);
        if (mx->kind[i] == 0 && mx->buf_len[i] > 0 && !mx->buf_scratch[i])
            return fail(THRL_ERR_NULL, "agent %d: QTable agents need buf_scratch", i);
        a.kind[i] = mx->kind[i]; a.nn_params[i] = mx->nn_params[i];
        a.buf_price[i] = mx->buf_price[i]; a.buf_action[i] = mx->buf_action[i]; a.buf_reward[i] = mx->buf_reward[i];
        a.buf_nprice[i] = mx->buf_nprice[i]; a.buf_ov[i] = mx->buf_scratch[i];
        a.buf_len[i] = mx->buf_len[i]; a.min_memory[i] = mx->min_memory[i]; a.count0[i] = mx->count[i];
        a.eps0[i] = run->eps[i];
    }
    if ((mx->sweep_eps_end || mx->sweep_eps_step) && !mx->sweep_eps)
        return fail(THRL_ERR_NULL, "sweep_eps_end / sweep_eps_step need the per-game epsilon state sweep_eps");
    if (mx->sweep_noise_prob && !(c->noise_prob > 0.0))
        return fail(THRL_ERR_BAD_CONFIG, "sweep_noise_prob needs cfg.noise_prob > 0 (it switches the noise draws on)");
    a.sw_gamma = mx->sweep_gamma; a.sw_alpha = mx->sweep_alpha; a.sw_eps_end = mx->sweep_eps_end;
    a.sw_eps_step = mx->sweep_eps_step; a.sw_eps = mx->sweep_eps; a.sw_noise_prob = mx->sweep_noise_prob;
    // ---- parity mode: all or nothing -- every stream this game consumes must be given
    const bool injected = mx->inj_u || mx->inj_choice || mx->inj_noise_u || mx->inj_noise_a || mx->inj_action;
    if (injected) {
        bool has_q = false, has_policy = false;
        for (int i = 0; i < c->n_agents; i++) {
            if (mx->kind[i] == 3)
                return fail(THRL_ERR_UNSUPPORTED, "agent %d: a CAC agent cannot play from injected draws (its action is a float)", i);
            if (mx->kind[i] == 0) has_q = true; else has_policy = true;
        }
        if (has_q && (!mx->inj_u || !mx->inj_choice))
            return fail(THRL_ERR_BAD_CONFIG, "injection: a QTable agent needs inj_u and inj_choice");
        if (has_policy && !mx->inj_action)
            return fail(THRL_ERR_BAD_CONFIG, "injection: a Reinforce / ActorCritic agent needs inj_action");
        if (c->noise_prob > 0.0 && (!mx->inj_noise_u || !mx->inj_noise_a))
            return fail(THRL_ERR_BAD_CONFIG, "injection: noise_prob > 0 needs inj_noise_u and inj_noise_a");
        a.inj = 1;
        a.inj_u = mx->inj_u; a.inj_choice = mx->inj_choice; a.inj_action = mx->inj_action;
        a.inj_noise_u = mx->inj_noise_u; a.inj_noise_a = mx->inj_noise_a;
    }
    // ---- two-agent games with discrete policies, noise-free: the tuple-chain kernel (thrl_ptuple.hip), same results
    {
        PTuplePlan tp = plan_ptuple(c, mx);
        if (tp.ok && mx->policy_tab && mx->policy_tab_bytes >= tp.scratch_bytes && !(mx->flags & THRL_MIXED_NO_TUPLE_KERNEL)) {
            PTupleArgs& t = tp.a;
            t.G = c->n_games; t.n_episodes = run->n_episodes; t.stride = a.stride;
            t.env = a.env;
            for (int i = 0; i < 2; i++) {
                t.ag[i] = a.ag[i];
                t.nn_params[i] = a.nn_params[i]; t.nn_stride[i] = a.nn_stride[i];
                t.buf_price[i] = a.buf_price[i]; t.buf_action[i] = a.buf_action[i]; t.buf_reward[i] = a.buf_reward[i];
                t.buf_nprice[i] = a.buf_nprice[i]; t.buf_len[i] = a.buf_len[i]; t.count0[i] = a.count0[i];
                t.eps0[i] = a.eps0[i];
            }
            t.q = q; t.counter = counter; t.state = state;
            t.sw_gamma = mx->sweep_gamma; t.sw_alpha = mx->sweep_alpha; t.sw_eps_end = mx->sweep_eps_end;
            t.sw_eps_step = mx->sweep_eps_step; t.sw_eps = mx->sweep_eps; t.sw_noise_prob = mx->sweep_noise_prob;
            t.inj = a.inj; t.inj_u = a.inj_u; t.inj_choice = a.inj_choice; t.inj_action = a.inj_action;
            t.inj_noise_u = a.inj_noise_u; t.inj_noise_a = a.inj_noise_a;
            unsigned char* base = (unsigned char*)mx->policy_tab;
            t.lut = base;
            t.next_game = (int32_t*)(base + kPTupleLutRegion - 64);
            t.policy_tab = (float*)(base + kPTupleLutRegion);
            t.game_reward_log = game_reward_log; t.game_action_log = game_action_log;
            t.seed = run->seed; t.game_offset = run->game_offset; t.first_episode = run->first_episode;
            t.waves_per_block = tp.waves_per_block;
            int grid = (c->n_games + tp.waves_per_block - 1) / tp.waves_per_block;
            const int max_grid = dev_info().cus * tp.blocks_per_cu;
            if (grid > max_grid) grid = max_grid;
            const size_t lds = (size_t)t.lut_lds_bytes + (size_t)tp.waves_per_block * t.game_lds_bytes;
            hipStream_t s = (hipStream_t)stream;
            int e = launch_ptuple_lut(t, base, s);
            if (e) return hip_fail(e, "k_ptuple_lut launch");
            if (hipMemsetAsync(t.next_game, 0, sizeof(int32_t), s) != hipSuccess) return hip_fail((int)hipGetLastError(), "hipMemsetAsync");
            e = launch_ptuple(t, c->q_dtype, grid, tp.waves_per_block * 64, lds, s);
            if (e) return hip_fail(e, "k_ptuple_episodes launch");
            run->kernel_used = THRL_KERNEL_TUPLE;
            goto bookkeeping;
        }
    }
    a.policy_tab = mx->policy_tab; a.policy_tab_bytes = mx->policy_tab ? mx->policy_tab_bytes : 0;
    {
    const char* why = "";
    if (plan_mixed(a, c->q_dtype, &why)) return fail(THRL_ERR_UNSUPPORTED, "thrl_mixed_episodes: %s", why);
    const int e = launch_mixed(a, c->q_dtype, (hipStream_t)stream);
    if (e) return hip_fail(e, "k_mixed_episodes launch");
    }
bookkeeping:
    // host mirror of the bookkeeping that is identical for every game
    for (int ep = 0; ep < run->n_episodes; ep++)
        for (int i = 0; i < c->n_agents; i++) {
            const int cap = mx->buf_len[i];
            if (cap > 0)
                for (int t = 0; t < c->max_steps; t++) {
                    mx->count[i] += 1;
                    if (mx->count[i] >= 2 * cap) mx->count[i] -= cap;
                }
            if (mx->kind[i] == 0) {
                const int len = mx->count[i] < cap ? mx->count[i] : cap;
                if (cap > 0 && len >= mx->min_memory[i]) mx->count[i] = 0;
                run->eps[i] = c->eps_end[i] + (run->eps[i] - c->eps_end[i]) * c->eps_step[i];
            }
        }
    return THRL_OK;
}

size_t thrl_mixed_policy_table_bytes(const thrl_cfg* c, const thrl_mixed* mx) {
    if (validate(c) != THRL_OK || !mx) return 0;
    MixedArgs a;
    memset(&a, 0, sizeof(a));
    a.G = c->n_games; a.N = c->n_agents; a.T = c->max_steps;
    fill_agents(c, a.ag, &a.env);
    for (int i = 0; i < c->n_agents; i++) {
        if (mx->kind[i] < 0 || mx->kind[i] > 3) return 0;
        a.kind[i] = mx->kind[i];
    }
    const char* why = "";
    size_t need = 0;
    if (plan_mixed(a, c->q_dtype, &why) == 0 && a.ptab_tuples > 0) need = a.ptab_need_bytes;
    // the tuple-chain kernel keeps its LUT image (and, against a QTable, its CDF rows) in the same scratch; buffer
    // state (count) does not change the size
    thrl_mixed probe = *mx;
    for (int i = 0; i < c->n_agents && i < THRL_MAXA; i++) probe.count[i] = 0;
    const PTuplePlan tp = plan_ptuple(c, &probe);
    if (tp.ok && tp.scratch_bytes > need) need = tp.scratch_bytes;
    return need;
}

int thrl_cac_init(int n_games, float* params, uint64_t seed, uint64_t game_offset, int agent, void* stream) {
    if (n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", n_games);
    if (!params) return fail(THRL_ERR_NULL, "params is NULL");
    const int e = launch_cac_init(n_games, params, seed, game_offset, agent, (hipStream_t)stream);
    return e ? hip_fail(e, "k_cac_init launch") : THRL_OK;
}

int thrl_cac_act(int n_games, const float* params, const double* price, const double* u1, const double* u2,
                 float* action_out, float* mu_out, float* std_out, float* v_out, void* stream) {
    if (n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", n_games);
    if (!params || !price || !action_out) return fail(THRL_ERR_NULL, "params/price/action_out is NULL");
    if ((u1 == nullptr) != (u2 == nullptr)) return fail(THRL_ERR_NULL, "u1 and u2 must both be given or both NULL");
    const int e = launch_cac_act(n_games, params, price, u1, u2, action_out, mu_out, std_out, v_out, (hipStream_t)stream);
    return e ? hip_fail(e, "k_cac_act launch") : THRL_OK;
}

int thrl_cac_train(int n_games, float* params, float* adam_m, float* adam_v, int32_t step, int32_t n, int32_t ld,
                   const double* price, const float* action, const double* reward, const double* next_price,
                   double gamma, double entropy_coef, double lr, const double* sweep_gamma, const double* sweep_entropy,
                   float* grad_out, void* stream) {
    if (n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", n_games);
    if (!params || !adam_m || !adam_v || !price || !action || !reward || !next_price)
        return fail(THRL_ERR_NULL, "a required pointer is NULL");
    if (n < 2 || cac_train_lds_bytes(n) > 160 * 1024)
        return fail(THRL_ERR_UNSUPPORTED, "n=%d transitions: need 2 <= n and the batch in LDS (n <= ~5600)", n);
    if (step < 0) return fail(THRL_ERR_BAD_CONFIG, "step < 0");
    if (ld < n) return fail(THRL_ERR_BAD_CONFIG, "ld=%d < n=%d", ld, n);
    const int e = launch_cac_train(n_games, params, adam_m, adam_v, step, n, ld, price, action, reward, next_price,
                                   (float)gamma, (float)entropy_coef, (float)lr, sweep_gamma, sweep_entropy, grad_out,
                                   (hipStream_t)stream);
    return e ? hip_fail(e, "k_cac_train launch") : THRL_OK;
}

int thrl_op_draws(const thrl_cfg* c, uint64_t seed, uint64_t game_offset, uint64_t episode, int32_t step,
                  double* u_out, int8_t* choice_out, double* u2_out, double* noise_u_out, double* noise_a_out,
                  void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!u_out || !choice_out) return fail(THRL_ERR_NULL, "u_out/choice_out is NULL");
    if ((noise_u_out == nullptr) != (noise_a_out == nullptr)) return fail(THRL_ERR_NULL, "noise outputs must both be given or both NULL");
    int32_t nA[THRL_MAXA];
    for (int i = 0; i < THRL_MAXA; i++) nA[i] = i < c->n_agents ? c->n_actions[i] : 1;
    const int e = launch_op_draws(c->n_games, c->n_agents, seed, game_offset, (uint32_t)episode, (uint32_t)step,
                                  c->env_a, c->env_a * 0.7, nA, u_out, choice_out, u2_out, noise_u_out, noise_a_out,
                                  (hipStream_t)stream);
    return e ? hip_fail(e, "k_op_draws launch") : THRL_OK;
}

int thrl_group_stats(const thrl_group_stats_args* g, void* stream) {
    if (!g) return fail(THRL_ERR_NULL, "args is NULL");
    if (g->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", g->n_games);
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
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
    if (x->deviator < 0 || x->deviator >= N)
        return fail(THRL_ERR_BAD_CONFIG, "deviator=%d out of [0,%d)", x->deviator, N);
    if (x->dev_len < 1) return fail(THRL_ERR_BAD_CONFIG, "dev_len=%d must be >= 1", x->dev_len);
    if (x->n_steps < x->dev_len || x->n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [dev_len=%d, %d]", x->n_steps, x->dev_len, THRL_DEV_MAX_STEPS);
    if (x->horizon < 1 || x->horizon > THRL_DEV_MAX_HORIZON)
        return fail(THRL_ERR_BAD_CONFIG, "horizon=%d out of [1,%d]", x->horizon, THRL_DEV_MAX_HORIZON);
    if (x->dev_action < -1 || x->dev_action >= c->n_actions[x->deviator])
        return fail(THRL_ERR_BAD_CONFIG, "dev_action=%d: -1 (best response) or an action of agent %d in [0,%d)",
                    x->dev_action, x->deviator, c->n_actions[x->deviator]);
    if (x->row_begin < 0 || x->row_count < 0 || (int64_t)x->row_begin + x->row_count > x->n_steps)
        return fail(THRL_ERR_BAD_CONFIG, "rows [%d, %d + %d) outside [0, n_steps=%d)", x->row_begin, x->row_begin,
                    x->row_count, x->n_steps);
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
    int lo[THRL_MAXA], hi[THRL_MAXA];
    reach_window(c, lo, hi);
    int entries = 0, lut_n = 0, max_a = 0;
    for (int i = 0; i < N; i++) {
        a.win_lo[i] = lo[i];
        a.win_n[i] = hi[i] - lo[i] + 1;
        a.pol_off[i] = entries;
        entries += a.win_n[i] + 1;                   // + x_0's row
        a.lut_off[i] = lut_n;
        lut_n += c->n_actions[i];
        if (c->n_actions[i] > max_a) max_a = c->n_actions[i];
    }
    a.pol_off[N] = entries;
    a.pol_entries = entries;
    a.lut_n = lut_n;
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
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
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
    int P = 0;
    for (int i = 0; i < N; i++) {
        a.row_off[i] = P;
        a.table_off[i] = ag[i].table_off;
        a.n_actions[i] = ag[i].n_actions;
        P += ag[i].rows;
    }
    a.row_off[N] = P;
    a.P = P;
    // the staged window: the game's block widened to 16-byte chunks at both ends
    const int64_t esz = c->q_dtype == 1 ? 8 : 4, vec = 16 / esz;
    const int64_t lds = ((a.stride + 2 * vec) * esz + 15) & ~(int64_t)15;
    a.staged = lds <= kTrackLdsBudget && ((uintptr_t)q & 15) == 0;
    a.lds_bytes = a.staged ? (int32_t)lds : 0;
    a.q = q; a.policy = x->policy; a.stable_since = x->stable_since; a.converged_at = x->converged_at;
    a.conv_since = x->conv_since; a.changes = x->changes; a.n_converged = x->n_converged;
    a.state = x->state; a.q_conv = x->q_conv; a.state_conv = x->state_conv;
    // enough one-wave blocks to fill every CU as far as LDS allows, each looping over games
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    int per_cu = kTrackMaxBlocksPerCu;
    if (a.staged && lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
    const int e = thrl::launch_policy_track(a, c->q_dtype, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_policy_track launch") : THRL_OK;
}

// The greedy policy of the first G games of q into policy [G][P], 2 bytes per table row (k_xplay_extract): the pass
// thrl_crossplay and thrl_attractors run without their POLICY_GIVEN flag.
static int extract_policies(const thrl_cfg* c, const void* q, int G, uint16_t* policy, void* stream) {
    const int N = c->n_agents;
    AgentParams ag[THRL_MAXA];
    fill_agents(c, ag, nullptr);
    XpExtractArgs e;
    memset(&e, 0, sizeof(e));
    int P = 0;
    for (int i = 0; i < N; i++) {
        e.row_off[i] = P;
        e.table_off[i] = ag[i].table_off;
        e.n_actions[i] = ag[i].n_actions;
        P += ag[i].rows;
    }
    e.row_off[N] = P;
    e.G = G; e.N = N; e.P = P;
    e.stride = (int64_t)thrl_table_stride(c);
    // the staged window: the game's block widened to 16-byte chunks at both ends
    const int64_t esz = c->q_dtype == 1 ? 8 : 4, vec = 16 / esz;
    const int64_t lds = ((e.stride + 2 * vec) * esz + 15) & ~(int64_t)15;
    e.staged = lds <= kXpExtractLdsBudget && ((uintptr_t)q & 15) == 0;
    e.lds_bytes = e.staged ? (int32_t)lds : 0;
    e.q = q; e.policy = policy;
    // enough one-wave blocks to fill every CU as far as LDS allows, each looping over games
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    int per_cu = kXpExtractMaxBlocksPerCu;
    if (e.staged && lds_cu > 0 && lds_cu / e.lds_bytes < per_cu) per_cu = lds_cu / e.lds_bytes > 0 ? lds_cu / e.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < e.G ? want : e.G);
    const int err = thrl::launch_xplay_extract(e, c->q_dtype, grid, (hipStream_t)stream);
    return err ? hip_fail(err, "k_xplay_extract launch") : THRL_OK;
}

int thrl_crossplay(const thrl_cfg* c, const void* q, const thrl_crossplay_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if (x->n_matches < 1) return fail(THRL_ERR_BAD_CONFIG, "n_matches=%d must be >= 1", x->n_matches);
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
    if (x->horizon < 1 || x->horizon > THRL_DEV_MAX_HORIZON)
        return fail(THRL_ERR_BAD_CONFIG, "horizon=%d out of [1,%d]", x->horizon, THRL_DEV_MAX_HORIZON);
    if (x->n_steps < 0 || x->n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [0,%d]", x->n_steps, THRL_DEV_MAX_STEPS);
    if (x->row_begin < 0 || x->row_count < 0 || (int64_t)x->row_begin + x->row_count > x->n_steps)
        return fail(THRL_ERR_BAD_CONFIG, "rows [%d, %d + %d) outside [0, n_steps=%d)", x->row_begin, x->row_begin,
                    x->row_count, x->n_steps);
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
    int P = 0, row_off[THRL_MAXA + 1];
    for (int i = 0; i < N; i++) { row_off[i] = P; P += ag[i].rows; }
    row_off[N] = P;

    if (!given) {       // one streaming pass over q: policy[g] for every g < G
        if ((rc = extract_policies(c, q, x->n_games, x->policy, stream)) != THRL_OK) return rc;
    }

    XpWalkArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.M = x->n_matches; a.N = N; a.P = P; a.H = x->horizon; a.K = x->n_steps;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    a.env = env;
    int lo[THRL_MAXA], hi[THRL_MAXA];
    reach_window(c, lo, hi);
    int entries = 0, lut_n = 0;
    for (int i = 0; i < N; i++) {
        a.ag[i] = ag[i];
        a.row_off[i] = row_off[i];
        a.win_lo[i] = lo[i];
        a.win_n[i] = hi[i] - lo[i] + 1;
        a.pol_off[i] = entries;
        entries += a.win_n[i] + 1;                   // + x_0's row
        a.lut_off[i] = lut_n;
        lut_n += c->n_actions[i];
    }
    a.pol_off[N] = entries;
    a.pol_entries = entries;
    a.lut_n = lut_n;
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
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->price || !x->tuple_policy) return fail(THRL_ERR_NULL, "price / tuple_policy is NULL");
    return extract_at_prices(c, q, x->kind, x->nn_params, x->n_games, x->n_tuples, x->price, 0, x->tuple_policy, stream);
}

int thrl_price_policy(const thrl_cfg* c, const void* q, const thrl_price_policy_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
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
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->horizon < 1 || x->horizon > THRL_DEV_MAX_HORIZON)
        return fail(THRL_ERR_BAD_CONFIG, "horizon=%d out of [1,%d]", x->horizon, THRL_DEV_MAX_HORIZON);
    if (x->n_steps < 0 || x->n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [0,%d]", x->n_steps, THRL_DEV_MAX_STEPS);
    if (x->row_begin < 0 || x->row_count < 0 || (int64_t)x->row_begin + x->row_count > x->n_steps)
        return fail(THRL_ERR_BAD_CONFIG, "rows [%d, %d + %d) outside [0, n_steps=%d)", x->row_begin, x->row_begin,
                    x->row_count, x->n_steps);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->seat || !x->start || !x->tuple_policy || !x->reward || !x->scaled || !x->mu || !x->lam || !x->cycle_reward
        || !x->cycle_action)
        return fail(THRL_ERR_NULL, "seat / start / tuple_policy / reward / scaled / mu / lam / cycle_reward / cycle_action is NULL");
    TpWalkArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.M = x->n_matches; a.N = N; a.T = x->n_tuples; a.H = x->horizon; a.K = x->n_steps;
    a.row_begin = x->row_begin; a.row_count = x->row_count;
    int stride = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = stride;
        stride *= c->n_actions[i];
    }
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
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->deviator < 0 || x->deviator >= N)
        return fail(THRL_ERR_BAD_CONFIG, "deviator=%d out of [0,%d)", x->deviator, N);
    if (x->dev_len < 1) return fail(THRL_ERR_BAD_CONFIG, "dev_len=%d must be >= 1", x->dev_len);
    if (x->n_steps < x->dev_len || x->n_steps > THRL_DEV_MAX_STEPS)
        return fail(THRL_ERR_BAD_CONFIG, "n_steps=%d out of [dev_len=%d, %d]", x->n_steps, x->dev_len, THRL_DEV_MAX_STEPS);
    if (x->horizon < 1 || x->horizon > THRL_DEV_MAX_HORIZON)
        return fail(THRL_ERR_BAD_CONFIG, "horizon=%d out of [1,%d]", x->horizon, THRL_DEV_MAX_HORIZON);
    if (x->dev_action < -1 || x->dev_action >= c->n_actions[x->deviator])
        return fail(THRL_ERR_BAD_CONFIG, "dev_action=%d: -1 (best response) or an action of agent %d in [0,%d)",
                    x->dev_action, x->deviator, c->n_actions[x->deviator]);
    if (x->row_begin < 0 || x->row_count < 0 || (int64_t)x->row_begin + x->row_count > x->n_steps)
        return fail(THRL_ERR_BAD_CONFIG, "rows [%d, %d + %d) outside [0, n_steps=%d)", x->row_begin, x->row_begin,
                    x->row_count, x->n_steps);
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
    int stride = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = stride;
        stride *= c->n_actions[i];
    }
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
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->agents == 0 || (x->agents & ~((1 << N) - 1)))
        return fail(THRL_ERR_BAD_CONFIG, "agents=0x%x: a non-empty mask of agents in [0,%d)", x->agents, N);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (!x->sweep_gamma)
        for (int i = 0; i < N; i++)
            if (((x->agents >> i) & 1) && !(c->gamma[i] >= 0.0 && c->gamma[i] < 1.0))
                return fail(THRL_ERR_BAD_CONFIG, "agent %d: gamma=%g: the equilibrium check needs gamma in [0, 1)", i,
                            c->gamma[i]);
    if (!x->start || !x->tuple_policy || !x->reward || !x->mu || !x->lam || !x->iters || !x->n_diff_all
        || !x->n_diff_on || !x->loss_all || !x->loss_on || !x->loss_all_mean || !x->loss_on_mean || !x->v_on)
        return fail(THRL_ERR_NULL, "start / tuple_policy / reward / mu / lam / iters / n_diff_all / n_diff_on / loss_all / "
                                   "loss_on / loss_all_mean / loss_on_mean / v_on is NULL");
    TaEqArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.agents = x->agents;
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = ts;
        ts *= c->n_actions[i];
        a.gamma[i] = c->gamma[i];
    }
    // LDS of a block: 8-byte arrays first, then 2-byte (each padded to 16 bytes), then the fixed words: at most
    // kTaEqLdsPerTuple * T + kTaEqLdsFixed + 144 bytes, 144.3 KB at T = 4096, whatever N is
    const int T = a.T;
    const int b8 = (8 * T + 15) & ~15, b2 = (2 * T + 15) & ~15;
    int off = 0;
    a.o_va = off; off += b8;
    a.o_vb = off; off += b8;
    a.o_rew = off; off += b8;
    a.o_na = off; off += b2;
    a.o_nb = off; off += b2;
    a.o_sigma = off; off += b2;
    a.o_jn = off; off += b2;
    a.o_mark = off; off += b2;
    a.o_base = off; off += b2;
    a.o_misc = off; off += kTaEqLdsFixed;
    a.lds_bytes = off;
    a.start = x->start; a.policy = x->tuple_policy; a.reward = x->reward; a.sweep_gamma = x->sweep_gamma;
    a.mu = x->mu; a.lam = x->lam; a.iters = x->iters; a.n_diff_all = x->n_diff_all; a.n_diff_on = x->n_diff_on;
    a.loss_all = x->loss_all; a.loss_on = x->loss_on; a.loss_all_mean = x->loss_all_mean;
    a.loss_on_mean = x->loss_on_mean; a.v_on = x->v_on;
    a.br_policy = x->br_policy; a.v_opt = x->v_opt; a.v_pi = x->v_pi;
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within THRL_TP_MAX_TUPLES
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_equilibrium: %d bytes of LDS per game, the device has %d", a.lds_bytes, lds_cu);
    int per_cu = kTaEqMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
    const int e = thrl::launch_ta_equilibrium(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ta_equilibrium launch") : THRL_OK;
}

int thrl_tuple_attractors(const thrl_cfg* c, const thrl_tuple_attractors_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
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
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = ts;
        ts *= c->n_actions[i];
    }
    // LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte (each padded to 16 bytes): kTatLdsPerTuple * T plus
    // the staging of a chunk of start weights, (8 * (1 + N) + 2) * kTatBlock bytes, and under 1 KB of fixed words:
    // 102.7 KB at T = 4096 with two agents, 115.1 KB with eight
    const int T = a.T;
    const int b4 = (4 * T + 15) & ~15, b2 = (2 * T + 15) & ~15;
    int off = 0;
    a.o_cw = off; off += 8 * kTatBlock;
    a.o_cprod = off; off += 8 * kTatBlock * N;
    a.o_cmean = off; off += 8 * THRL_ATTR_KEEP * N;
    a.o_basin = off; off += b4;
    a.o_lamc = off; off += b4;
    a.o_sel = off; off += 4 * THRL_ATTR_KEEP;
    a.o_red = off; off += 4 * 20;
    off = (off + 15) & ~15;
    a.o_f = off; off += b2;
    a.o_pa = off; off += b2;
    a.o_pb = off; off += b2;
    a.o_ma = off; off += b2;
    a.o_mb = off; off += b2;
    a.o_rep = off; off += b2;
    a.o_on = off; off += b2;
    a.o_slot = off; off += b2;
    a.o_cslot = off; off += 2 * kTatBlock;
    a.lds_bytes = off;
    a.start = x->start; a.policy = x->tuple_policy; a.reward = x->reward; a.scaled = x->scaled; a.start_w = x->start_w;
    a.n_attr = x->n_attr; a.mu_max = x->mu_max; a.n_cycle_states = x->n_cycle_states;
    a.rep = x->rep; a.lam = x->lam; a.basin = x->basin; a.cycle_reward = x->cycle_reward; a.cycle_action = x->cycle_action;
    a.rep_x0 = x->rep_x0; a.mu_x0 = x->mu_x0; a.slot_x0 = x->slot_x0;
    a.start_mass = x->start_mass; a.start_mass_other = x->start_mass_other; a.start_reward = x->start_reward;
    a.tuple_rep = x->tuple_rep; a.tuple_mu = x->tuple_mu;
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within THRL_TP_MAX_TUPLES
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_attractors: %d bytes of LDS per game, the device has %d", a.lds_bytes, lds_cu);
    int per_cu = kTatMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
    const int e = thrl::launch_tuple_attractors(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ta_attractors launch") : THRL_OK;
}

int thrl_tuple_stationary(const thrl_cfg* c, const thrl_tuple_stationary_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked before the device is touched
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->flags & ~THRL_TS_START_TUPLE) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (x->n_cells < 1 || x->band_w < 1)
        return fail(THRL_ERR_BAD_CONFIG, "n_cells=%d and band_w=%d must be >= 1", x->n_cells, x->band_w);
    if (x->max_iters < 1 || x->max_iters > THRL_STAT_MAX_ITERS)
        return fail(THRL_ERR_BAD_CONFIG, "max_iters=%d out of [1,%d]", x->max_iters, THRL_STAT_MAX_ITERS);
    if (!(x->tol >= 0.0)) return fail(THRL_ERR_BAD_CONFIG, "tol=%g must be >= 0", x->tol);
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
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = ts;
        ts *= c->n_actions[i];
        if (x->kind[i] != 0) a.neural_mask |= 1 << i;
    }
    // LDS of a block (the working set of include/thrl.h): 8-byte arrays first, nu directly behind the second iterate,
    // then the 2-byte arrays of the two groupings
    const int T = a.T, J = a.J;
    int off = 0;
    a.o_ma = off; off += 8 * T;
    a.o_mb = off; off += 8 * T;
    a.o_nu = off; off += 8 * J;
    a.o_prod = off; off += 8 * 64 * (2 * N + 2);
    a.o_permk = off; off += 2 * J;
    a.o_startk = off; off += 2 * (T + 1);
    a.o_permt = off; off += 2 * T;
    a.o_startt = off; off += 2 * (T + 1);
    a.lds_bytes = (off + 15) & ~15;
    a.noise_prob_g = x->noise_prob_g; a.start = x->start; a.tuple_policy = x->tuple_policy; a.cell_policy = x->cell_policy;
    a.cell_w = x->cell_w; a.reward = x->reward; a.scaled = x->scaled; a.price = x->price; a.band_lo = x->band_lo;
    a.band = x->band; a.noise_reward = x->noise_reward; a.noise_price = x->noise_price;
    a.iters = x->iters; a.change = x->change; a.mass = x->mass; a.stat_reward = x->stat_reward;
    a.stat_action = x->stat_action; a.stat_price = x->stat_price; a.pi = x->pi;
    a.n_switch = x->n_switch; a.unresolved = x->unresolved;
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    if (lds_cu > 0 && a.lds_bytes > lds_cu)          // cannot happen on a 160 KB CU within the limits on T and J
        return fail(THRL_ERR_UNSUPPORTED, "thrl_tuple_stationary: %d bytes of LDS per game (T=%d, n_cells=%d), the device has %d",
                    a.lds_bytes, T, J, lds_cu);
    int per_cu = kTsMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
    const int e = thrl::launch_tuple_stationary(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_ts_switch / k_ts_chain launch") : THRL_OK;
}

int thrl_price_probs(const thrl_cfg* c, const thrl_price_probs_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
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

int thrl_sampled_chain(const thrl_cfg* c, const thrl_sampled_chain_args* x, void* stream) {
    int rc = validate(c);
    if (rc) return rc;
    if (!x) return fail(THRL_ERR_NULL, "args is NULL");
    const int N = c->n_agents;
    // every host-visible argument is checked before the device is touched
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->flags & ~THRL_SP_START_TUPLE) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (x->n_prices < 1 || x->n_prices > x->n_tuples)
        return fail(THRL_ERR_BAD_CONFIG, "n_prices=%d out of [1, n_tuples=%d]", x->n_prices, x->n_tuples);
    if (x->max_iters < 1 || x->max_iters > THRL_STAT_MAX_ITERS)
        return fail(THRL_ERR_BAD_CONFIG, "max_iters=%d out of [1,%d]", x->max_iters, THRL_STAT_MAX_ITERS);
    if (!(x->tol >= 0.0)) return fail(THRL_ERR_BAD_CONFIG, "tol=%g must be >= 0", x->tol);
    if (!x->eps_g)
        for (int i = 0; i < N; i++)
            if (x->kind[i] == 0 && !(x->eps[i] >= 0.0 && x->eps[i] <= 1.0))
                return fail(THRL_ERR_BAD_CONFIG, "eps[%d]=%g out of [0, 1]", i, x->eps[i]);
    SpArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = x->n_tuples; a.D = x->n_prices;
    a.max_iters = x->max_iters; a.start_tuple = (x->flags & THRL_SP_START_TUPLE) != 0;
    a.tol = x->tol;
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) {
        a.kind[i] = x->kind[i];
        a.n_actions[i] = c->n_actions[i];
        a.tstride[i] = ts;
        ts *= c->n_actions[i];
        a.eps[i] = x->eps[i];
        a.prob[i] = x->prob[i];
    }
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
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    if (lds_cu > 0 && a.lds_bytes > lds_cu)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_chain: %d bytes of LDS per game (T=%d, n_prices=%d), the device has %d",
                    a.lds_bytes, a.T, a.D, lds_cu);
    int per_cu = kSpMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
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
    if (x->n_games < 1) return fail(THRL_ERR_BAD_CONFIG, "n_games=%d must be >= 1", x->n_games);
    if (x->flags & ~(THRL_SPN_START_TUPLE | THRL_SPN_START_RESET)) return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if ((x->flags & THRL_SPN_START_TUPLE) && (x->flags & THRL_SPN_START_RESET))
        return fail(THRL_ERR_BAD_CONFIG, "THRL_SPN_START_TUPLE and THRL_SPN_START_RESET are both set");
    if (x->reserved != 0) return fail(THRL_ERR_BAD_CONFIG, "reserved=%d must be 0", x->reserved);
    if ((rc = tuple_kinds_check(c, x->kind)) != THRL_OK) return rc;
    if ((rc = tuple_count_check(c, x->n_tuples)) != THRL_OK) return rc;
    if (x->n_prices < 1 || x->n_prices > x->n_tuples)
        return fail(THRL_ERR_BAD_CONFIG, "n_prices=%d out of [1, n_tuples=%d]", x->n_prices, x->n_tuples);
    if (x->n_nodes < 2 || x->band_w < 1)
        return fail(THRL_ERR_BAD_CONFIG, "n_nodes=%d must be >= 2 and band_w=%d >= 1", x->n_nodes, x->band_w);
    if (x->max_iters < 1 || x->max_iters > THRL_STAT_MAX_ITERS)
        return fail(THRL_ERR_BAD_CONFIG, "max_iters=%d out of [1,%d]", x->max_iters, THRL_STAT_MAX_ITERS);
    if (!(x->tol >= 0.0)) return fail(THRL_ERR_BAD_CONFIG, "tol=%g must be >= 0", x->tol);
    if (!x->eps_g)
        for (int i = 0; i < N; i++)
            if (x->kind[i] == 0 && !(x->eps[i] >= 0.0 && x->eps[i] <= 1.0))
                return fail(THRL_ERR_BAD_CONFIG, "eps[%d]=%g out of [0, 1]", i, x->eps[i]);
    if (!x->noise_prob_g && !(x->noise_prob >= 0.0 && x->noise_prob <= 1.0))
        return fail(THRL_ERR_BAD_CONFIG, "noise_prob=%g out of [0, 1]", x->noise_prob);
    if (x->n_nodes > THRL_STAT_MAX_CELLS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_noise_chain: n_nodes=%d, at most %d", x->n_nodes, THRL_STAT_MAX_CELLS);
    thrl::SpnArgs a;
    memset(&a, 0, sizeof(a));
    SpArgs& sa = a.sp;
    sa.G = x->n_games; sa.N = N; sa.T = x->n_tuples; sa.D = x->n_prices;
    sa.max_iters = x->max_iters; sa.start_tuple = (x->flags & THRL_SPN_START_TUPLE) != 0;
    sa.tol = x->tol;
    a.Jn = x->n_nodes; a.W = x->band_w; a.start_reset = (x->flags & THRL_SPN_START_RESET) != 0;
    a.noise_prob = x->noise_prob;
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) {
        sa.kind[i] = x->kind[i];
        sa.n_actions[i] = c->n_actions[i];
        sa.tstride[i] = ts;
        ts *= c->n_actions[i];
        sa.eps[i] = x->eps[i];
        sa.prob[i] = x->prob[i];
        a.nprob[i] = x->nprob[i];
    }
    const int64_t lds = thrl::spn_layout(a);         // the working set of include/thrl.h
    if (lds > THRL_SP_MAX_LDS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_noise_chain: %lld bytes of LDS per game (T=%d, n_prices=%d, n_nodes=%d), at most %d",
                    (long long)lds, sa.T, sa.D, a.Jn, THRL_SP_MAX_LDS);
    for (int i = 0; i < N; i++)
        if (x->kind[i] != 0 && (!x->prob[i] || !x->nprob[i])) return fail(THRL_ERR_NULL, "prob[%d] / nprob[%d] is NULL", i, i);
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
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    if (lds_cu > 0 && sa.lds_bytes > lds_cu)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_sampled_noise_chain: %d bytes of LDS per game (T=%d, n_prices=%d, n_nodes=%d), the device has %d",
                    sa.lds_bytes, sa.T, sa.D, a.Jn, lds_cu);
    int per_cu = kSpMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / sa.lds_bytes < per_cu) per_cu = lds_cu / sa.lds_bytes > 0 ? lds_cu / sa.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < sa.G ? want : sa.G);
    const int e = thrl::launch_sampled_noise_chain(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_spn_jump / k_spn_chain launch") : THRL_OK;
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
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
    if (x->agents == 0 || (x->agents & ~((1 << N) - 1)))
        return fail(THRL_ERR_BAD_CONFIG, "agents=0x%x: a non-empty mask of agents in [0,%d)", x->agents, N);
    if (!x->sweep_gamma)
        for (int i = 0; i < N; i++)
            if (((x->agents >> i) & 1) && !(c->gamma[i] >= 0.0 && c->gamma[i] < 1.0))
                return fail(THRL_ERR_BAD_CONFIG, "agent %d: gamma=%g: the equilibrium check needs gamma in [0, 1)", i,
                            c->gamma[i]);
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
    int ts = 1;
    for (int i = N - 1; i >= 0; i--) { a.tstride[i] = ts; ts *= c->n_actions[i]; }
    // LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte
    const int S = h.S, T = h.T;
    const int64_t fixed = 3 * 8 * (int64_t)S + 4 * (int64_t)S + 4 * THRL_MAXA
                          + 2 * ((int64_t)T + (int64_t)N * S + THRL_MAXA + 5 * (int64_t)S) + 64;
    a.lut_lds = fixed + 8 * (int64_t)N * T <= kEqLdsBudget;
    int off = 0;
    a.o_va = off; off += 8 * S;
    a.o_vb = off; off += 8 * S;
    a.o_vpi = off; off += 8 * S;
    a.o_rew = off; off += a.lut_lds ? 8 * N * T : 0;
    a.o_base = off; off += 4 * S;
    a.o_x0row = off; off += 4 * THRL_MAXA;
    a.o_sid = off; off += 2 * T;
    a.o_first = off; off += 2 * S;
    a.o_pol = off; off += 2 * (N * S + THRL_MAXA);
    a.o_sigma = off; off += 2 * S;
    a.o_jn = off; off += 2 * S;
    a.o_na = off; off += 2 * S;
    a.o_nb = off; off += 2 * S;
    a.lds_bytes = (off + 15) & ~15;
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
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    int per_cu = kEqMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
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
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
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
    int ts = 1, P = 0;
    for (int i = N - 1; i >= 0; i--) { a.tstride[i] = ts; ts *= c->n_actions[i]; }
    for (int i = 0; i < N; i++) { a.row_off[i] = P; P += a.ag[i].rows; }
    a.P = P;
    // LDS of a block: 8-byte arrays first, then 4-byte, then 2-byte
    const int64_t fixed = 8 * 64 * (int64_t)(1 + N) + 4 * (2 * (int64_t)S + THRL_MAXA + THRL_ATTR_KEEP + 64)
                          + 2 * ((int64_t)T + (int64_t)N * S + THRL_MAXA + (int64_t)(a.L + 1) * S + 7 * (int64_t)S) + 64;
    a.lut_lds = fixed + 8 * (int64_t)N * T <= kAttrLdsBudget;
    if (fixed > kAttrLdsBudget)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_attractors: %lld bytes of LDS per game (N=%d, S=%d, T=%d)", (long long)fixed,
                    N, S, T);
    int off = 0;
    a.o_rew = off; off += a.lut_lds ? 8 * N * T : 0;
    a.o_cw = off; off += 8 * 64;
    a.o_cprod = off; off += 8 * 64 * N;
    a.o_basin = off; off += 4 * S;
    a.o_lamc = off; off += 4 * S;
    a.o_x0row = off; off += 4 * THRL_MAXA;
    a.o_sel = off; off += 4 * THRL_ATTR_KEEP;
    a.o_cslot = off; off += 4 * 64;
    a.o_sid = off; off += 2 * T;
    a.o_pol = off; off += 2 * (N * S + THRL_MAXA);
    a.o_lev = off; off += 2 * (a.L + 1) * S;
    a.o_ma = off; off += 2 * S;
    a.o_mb = off; off += 2 * S;
    a.o_rep = off; off += 2 * S;
    a.o_mu = off; off += 2 * S;
    a.o_on = off; off += 2 * S;
    a.o_tup = off; off += 2 * S;
    a.o_slot = off; off += 2 * S;
    a.lds_bytes = (off + 15) & ~15;

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
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    int per_cu = kAttrMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
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
    int64_t T64 = 1;
    for (int i = 0; i < N; i++) {
        T64 *= c->n_actions[i];
        if (T64 > THRL_EQ_MAX_TUPLES)
            return fail(THRL_ERR_UNSUPPORTED, "thrl_stationary: more than %d action tuples (prod n_actions)",
                        THRL_EQ_MAX_TUPLES);
    }
    const int T = (int)T64;
    if (x->n_tuples) *x->n_tuples = T;
    if (x->n_games < 1 || x->n_games > c->n_games)
        return fail(THRL_ERR_BAD_CONFIG, "n_games=%d out of [1,%d]", x->n_games, c->n_games);
    if (x->flags & ~(THRL_STAT_POLICY_GIVEN | THRL_STAT_START_STATE))
        return fail(THRL_ERR_BAD_CONFIG, "unknown flags 0x%x", x->flags);
    if (x->n_cells < 1 || x->band_w < 1)
        return fail(THRL_ERR_BAD_CONFIG, "n_cells=%d and band_w=%d must be >= 1", x->n_cells, x->band_w);
    if (x->max_iters < 1 || x->max_iters > THRL_STAT_MAX_ITERS)
        return fail(THRL_ERR_BAD_CONFIG, "max_iters=%d out of [1,%d]", x->max_iters, THRL_STAT_MAX_ITERS);
    if (!(x->tol >= 0.0)) return fail(THRL_ERR_BAD_CONFIG, "tol=%g must be >= 0", x->tol);
    if (!x->noise_prob_g && !(x->noise_prob > 0.0 && x->noise_prob <= 1.0))
        return fail(THRL_ERR_BAD_CONFIG, "noise_prob=%g out of (0, 1]", x->noise_prob);
    if (x->n_cells > THRL_STAT_MAX_CELLS)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_stationary: n_cells=%d, at most %d", x->n_cells, THRL_STAT_MAX_CELLS);
    // LDS of a block: the two iterates, the staging of the ordered sums and the tuple per cell must fit
    const int64_t J = x->n_cells;
    const int64_t need = 8 * 2 * J + 8 * 64 * (int64_t)(2 * N + 2) + 2 * J + 16;
    if (need > kStatLdsBudget)
        return fail(THRL_ERR_UNSUPPORTED, "thrl_stationary: %lld bytes of LDS per game (N=%d, n_cells=%d)", (long long)need,
                    N, x->n_cells);
    const bool given = (x->flags & THRL_STAT_POLICY_GIVEN) != 0;
    const bool start_state = (x->flags & THRL_STAT_START_STATE) != 0;
    if (!x->cell_rows || !x->cell_w || !x->det_cell || !x->band_lo || !x->band || !x->noise_reward || !x->noise_price)
        return fail(THRL_ERR_NULL, "cell_rows / cell_w / det_cell / band_lo / band / noise_reward / noise_price is NULL");
    if (!x->policy || !x->iters || !x->change || !x->mass || !x->stat_reward || !x->stat_action || !x->stat_price)
        return fail(THRL_ERR_NULL, "policy / iters / change / mass / stat_reward / stat_action / stat_price is NULL");
    if (start_state && !x->state0) return fail(THRL_ERR_NULL, "state0 is NULL with THRL_STAT_START_STATE");
    if (!given && !q) return fail(THRL_ERR_NULL, "q is NULL without THRL_STAT_POLICY_GIVEN");

    StatArgs a;
    memset(&a, 0, sizeof(a));
    a.G = x->n_games; a.N = N; a.T = T; a.J = x->n_cells; a.W = x->band_w;
    a.max_iters = x->max_iters; a.start_state = start_state;
    a.noise_prob = x->noise_prob; a.tol = x->tol;
    fill_agents(c, a.ag, &a.env);
    int ts = 1, P = 0;
    for (int i = N - 1; i >= 0; i--) { a.tstride[i] = ts; ts *= c->n_actions[i]; }
    for (int i = 0; i < N; i++) { a.row_off[i] = P; P += a.ag[i].rows; }
    a.P = P;
    // LDS layout: 8-byte arrays first, then 4-byte, then 2-byte
    a.cell_lds = need + 10 * J <= kStatLdsBudget;
    int off = 0;
    a.o_mua = off; off += 8 * a.J;
    a.o_mub = off; off += 8 * a.J;
    a.o_prod = off; off += 8 * 64 * (2 * N + 2);
    a.o_boff = off; off += a.cell_lds ? 4 * a.J : 0;
    a.o_blo = off; off += a.cell_lds ? 4 * a.J : 0;
    a.o_det = off; off += a.cell_lds ? 2 * a.J : 0;
    a.o_tup = off; off += 2 * a.J;
    a.lds_bytes = (off + 15) & ~15;
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
    int dev = 0, cus = 0, lds_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess
        || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
        || hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess)
        return hip_fail((int)hipGetLastError(), "device attributes");
    int per_cu = kStatMaxBlocksPerCu;
    if (lds_cu > 0 && lds_cu / a.lds_bytes < per_cu) per_cu = lds_cu / a.lds_bytes > 0 ? lds_cu / a.lds_bytes : 1;
    const int64_t want = (int64_t)(cus > 0 ? cus : 1) * per_cu;
    const int grid = (int)(want < a.G ? want : a.G);
    const int e = thrl::launch_stationary(a, grid, (hipStream_t)stream);
    return e ? hip_fail(e, "k_stationary launch") : THRL_OK;
}

}  // extern "C"
