// thrl_wave_kernel.h -- fused episode kernel for gfx950: ONE WAVEFRONT PER GAME (template body).
//
// The performance path for the reference's headline shape: 2 QTable agents with the same grid
// sizes on one NoisyPriceState.  Table type QT = float (the metric's dtype) or double (the
// reference's own numerics, agents.py:29).  Same semantics as thrl_generic.hip and bit-identical
// results to it and to the oracle in the same dtype: trainer.train_one's loop (th_rl/trainer.py:46-70)
// with QTable.sample_action (agents.py:80-89), scale (:51-57), NoisyPriceState.step
// (environments.py:25-39), ReplayBuffer append/replay/empty (buffers.py) and QTable.train_net
// (agents.py:59-78) fused, for `n_episodes` episodes per launch.
//
// MI355X mapping:
//   * a wave owns one game for the whole launch; its two agents' Q-table WINDOWS (only the rows the
//     payoff grid can reach, + 2 spill rows for an arbitrary initial state) are streamed coalesced
//     HBM -> LDS once, stay resident for all episodes of the launch, and are streamed back once;
//   * lanes 0-31 serve agent 0, lanes 32-63 agent 1;
//   * the discretised action grid (next-state row + price per action pair) is a LUT staged in LDS
//     once per block ("payoff LUT");
//   * everything that is not on a serial chain is done lane-parallel over the T steps of an episode
//     (lane = step) or over the table rows (lane = row): Philox draws, per-row greedy actions, reward /
//     old-value gathers, log sums, the replay schedule;
//   * play chain: s <- next_row_t[s], one v_readlane per step;
//   * replay (train_net's serial loop, agents.py:68-76) runs FOUR transitions per pass: each 32-lane
//     half is split into four 8-lane groups, group k reads the whole next-state row of transition
//     4g+k (3 columns per lane), one v_max3 + three DPP steps give every lane of the group that row's
//     max, and the lane holding transition 4g+k's operands computes the TD value and stores it.
//     A pass is legal when no transition in it reads a row, or rewrites a cell, that an earlier
//     transition of the same pass writes; the schedule (where a group of four must be cut into
//     several passes) is computed lane-parallel before the loop, so results are exactly those of the
//     serial loop.  The schedule also numbers every transition's pass (its "key"): a pass stores through the lanes
//     whose key matches (the compare writes EXEC), pass 0 of a group runs unconditionally, and one scalar test of
//     the group's cut bits finds the groups that need further passes -- no ranges, no ballots, no scalar loop
//     control in the hazard-free group;
//   * the kernel is bound by the number of instructions a wave issues, so the hot loops are
//     straight-line code: the play loop is unrolled over a segment's 16 groups of four steps and the replay
//     loop over a block's 8 groups (step / lane numbers are immediates), with copies for full segments and
//     full blocks that carry no bounds tests;
//   * log sums: an episode ends with one transposing reduction (wave_sum4) of its four totals.  The variants that keep
//     per-game rows (LOG) or play several episodes per training cycle (CYCLE) finish them there, per episode: divide by
//     T, scale to fixed point, round, add into the lane of that episode.  All others (the headline among them) only park
//     the four totals -- one 8-byte store by four lanes into the wave's `partial` region, which holds the launch's sums only
//     after the kernel's last two stores -- and the game's epilogue reads the region back with the transition log and
//     finishes all of the game's episodes lane-parallel in two passes (lane L: slot L into acc, slot 64 + L into acc_hi):
//     the same operations on the same doubles, once per lane and game instead of once per episode on a whole wave;
//   * GREEDY variants (launched once epsilon is small): groups of four steps in which nobody explores read
//     their next rows from per-episode composed tables, and a segment that cycles through 1-4 transitions
//     (a converged game) is replayed as a recurrence in registers (cyclic_segment).
#pragma once
#include <type_traits>
#include <utility>
#include "thrl_kernels.h"
#include "thrl_wave_lut.h"

// THRL_ABLATE: timing-only diagnostic builds (python -m th_rl_amd.build --ablate MASK, profiles/ablate.py).
// A set bit removes one phase of the kernel -- results are wrong by construction; the product library is
// always built with 0.  1 replay passes, 2 play chain, 4 play tables, 8 Philox, 16 per-row argmax,
// 32 visit counters (log + histogram), 64 log sums, 128 replay schedule.
#ifndef THRL_ABLATE
#define THRL_ABLATE 0
#endif

namespace thrl {

constexpr int kAblate = THRL_ABLATE;

typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// lanes<32 of the result: lanes 0-31 of a ; lanes>=32: lanes 0-31 of b   (.x)
// and the same for the upper halves (.y): one v_permlane32_swap.
__device__ __forceinline__ v2u pack_halves(unsigned a, unsigned b) {
    return __builtin_amdgcn_permlane32_swap(a, b, false, false);
}

// LDS access by 32-bit LDS address (address space 3): no generic-pointer arithmetic
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
template <typename QT>
__device__ __forceinline__ QT lds_load(unsigned addr) {
    typedef __attribute__((address_space(3))) QT lds_t;
    return *(const lds_t*)(uintptr_t)addr;
}
template <typename QT>
__device__ __forceinline__ void lds_store(unsigned addr, QT v) {
    typedef __attribute__((address_space(3))) QT lds_t;
    *(lds_t*)(uintptr_t)addr = v;
}

// The visit histogram overlays the tables: its accesses carry may_alias types (no type-based reordering against the
// tables' float / double accesses or against each other).
// += 1 on a u32 in LDS, no return value (ds_add_u32)
__device__ __forceinline__ void lds_inc(unsigned addr) {
    typedef unsigned __attribute__((may_alias)) u32_alias;
    typedef __attribute__((address_space(3))) u32_alias lds_u32;
    __hip_atomic_fetch_add((lds_u32*)(uintptr_t)addr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// 8 zero bytes at an 8-byte aligned LDS address (ds_write_b64)
__device__ __forceinline__ void lds_zero8(unsigned addr) {
    typedef unsigned long long __attribute__((may_alias)) u64_alias;
    typedef __attribute__((address_space(3))) u64_alias lds_u64;
    *(lds_u64*)(uintptr_t)addr = 0ull;
}

__device__ __forceinline__ unsigned bperm(unsigned byte_sel, unsigned v) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)byte_sel, (int)v);
}

// DPP move of a double (two dword moves)
template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false),
                            __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}

// max over each aligned group of 8 lanes, result in every lane of the group.
// float: three single-instruction DPP max steps (xor 1, xor 2 inside the quad, then the mirror of
// the 8-lane half row).  The s_nop 1 before each are the 2 wait states a DPP read of a just-written
// VGPR needs (hipcc does not look inside asm statements).
__device__ __forceinline__ float group8_allmax(float v) {
    asm("s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf"
        : "+v"(v));
    return v;
}
__device__ __forceinline__ double group8_allmax(double v) {
    v = fmax(v, dpp_mov64<0xB1>(v));       // quad_perm [1,0,3,2]
    v = fmax(v, dpp_mov64<0x4E>(v));       // quad_perm [2,3,0,1]
    v = fmax(v, dpp_mov64<0x141>(v));      // row_half_mirror
    return v;
}
// LDS store by the lanes of `mask` only, as straight-line code: hipcc turns `if (cond) store` into
// saveexec + skip branch + store + branch back; the mask is never empty here, so EXEC is simply swapped around
// the store.
__device__ __forceinline__ void store_where(unsigned long long mask, unsigned addr, float v) {
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b32 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "s"(mask), "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void store_where(unsigned long long mask, unsigned addr, double v) {
    unsigned long long save;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\tds_write_b64 %2, %3\n\ts_mov_b64 exec, %0"
                 : "=&s"(save) : "s"(mask), "v"(addr), "v"(v) : "memory");
}
// 8-byte global store by the lanes of `mask` only, to base + off (base and mask wave-uniform, off the lane's 32-bit byte
// offset), for code that is only reached with all 64 lanes active: EXEC is set by scalar moves, no compare, no save and
// no restore.  hipcc does not count the store (its s_waitcnt bookkeeping only gets more conservative by one), and
// nothing waits for it: the wave reads the word back through the same path, in order.
__device__ __forceinline__ void store_lanes(unsigned long long mask, long long* base, unsigned off, double v) {
    asm volatile("s_mov_b64 exec, %0\n\tglobal_store_dwordx2 %1, %2, %3\n\ts_mov_b64 exec, -1"
                 :: "s"(mask), "v"(off), "v"(v), "s"(base) : "memory");
}
// LDS store by the lanes whose replay key (phase (d2): 4 * group + pass number of the lane's transition) equals
// `want`, for code that is only reached with all 64 lanes active: the compare writes EXEC itself (v_cmpx; on gfx9 it
// writes VCC too) and EXEC is set back to all ones, no save and no restore.  No lane may match: the store then does
// nothing.  IMM >= 0: `want` as an inline constant (0..64), else the scalar `want`.
// Wait states (CDNA3/4 ISA guide, "manually inserted wait states"; hipcc does not look inside asm):
//   * "VALU writes EXEC -> VALU DPP op: 5": the next DPP operation is the row maximum of the next pass, behind this
//     store, the s_mov, that pass's row reads (>= 2), their s_waitcnt and a v_max: >= 6 states;
//   * "VALU writes SGPR/VCC -> v_readlane / v_writelane with that register as lane select: 4": no lane select in the
//     replay is VCC (immediates, or SGPRs written by the scalar unit);
//   * "VALU writes VCC -> v_div_fmas: 4": the replay has none.
// Neither the LDS store's use of the EXEC a VALU has just written nor the scalar write of EXEC has an entry.
template <int IMM>
__device__ __forceinline__ void store_key(unsigned key, unsigned want, unsigned addr, float v) {
    if constexpr (IMM >= 0)
        asm volatile("v_cmpx_eq_u32 vcc, %0, %1\n\tds_write_b32 %2, %3\n\ts_mov_b64 exec, -1"
                     :: "n"(IMM), "v"(key), "v"(addr), "v"(v) : "memory", "vcc");
    else
        asm volatile("v_cmpx_eq_u32 vcc, %0, %1\n\tds_write_b32 %2, %3\n\ts_mov_b64 exec, -1"
                     :: "s"(want), "v"(key), "v"(addr), "v"(v) : "memory", "vcc");
}
template <int IMM>
__device__ __forceinline__ void store_key(unsigned key, unsigned want, unsigned addr, double v) {
    if constexpr (IMM >= 0)
        asm volatile("v_cmpx_eq_u32 vcc, %0, %1\n\tds_write_b64 %2, %3\n\ts_mov_b64 exec, -1"
                     :: "n"(IMM), "v"(key), "v"(addr), "v"(v) : "memory", "vcc");
    else
        asm volatile("v_cmpx_eq_u32 vcc, %0, %1\n\tds_write_b64 %2, %3\n\ts_mov_b64 exec, -1"
                     :: "s"(want), "v"(key), "v"(addr), "v"(v) : "memory", "vcc");
}
// Packing of the key into the upper bits of a transition's LDS store address (a byte address below 2^18: 160 KB)
constexpr unsigned kKeyShift = 25;
constexpr unsigned kKeyNone = 0x7Fu;            // a transition that does not train: no pass has this key (passes: 0..31)
// the value of the lane 8 further on in the same 16-lane row (row_ror:8): swaps the two 8-lane groups of a row
__device__ __forceinline__ float dpp_ror8(float v) { return __builtin_bit_cast(float, dpp_mov32<0x128>(__builtin_bit_cast(uint32_t, v))); }
__device__ __forceinline__ double dpp_ror8(double v) { return dpp_mov64<0x128>(v); }
__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_of(double a, double b);
// max over each 32-lane half, result in every lane of the half: the 8-lane step above, the mirror of the 16-lane
// row, then the two rows of the half exchanged by v_permlane16_swap
__device__ __forceinline__ float half32_allmax(float v) {
    v = group8_allmax(v);
    v = fmaxf(v, __builtin_bit_cast(float, dpp_mov32<0x140>(__builtin_bit_cast(uint32_t, v))));      // row_mirror
    unsigned a = __builtin_bit_cast(unsigned, v), b = a;
    asm("" : "+v"(b));
    const v2u r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    const unsigned rx = r.x, ry = r.y;
    return fmaxf(__builtin_bit_cast(float, rx), __builtin_bit_cast(float, ry));
}
__device__ __forceinline__ double half32_allmax(double v) {
    v = group8_allmax(v);
    v = fmax(v, dpp_mov64<0x140>(v));
    unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    unsigned lo2 = lo, hi2 = hi;
    asm("" : "+v"(lo2), "+v"(hi2));
    const v2u rl = __builtin_amdgcn_permlane16_swap(lo, lo2, false, false);
    const v2u rh = __builtin_amdgcn_permlane16_swap(hi, hi2, false, false);
    const unsigned rlx = rl.x, rly = rl.y, rhx = rh.x, rhy = rh.y;
    return fmax(__hiloint2double((int)rhx, (int)rlx), __hiloint2double((int)rhy, (int)rly));
}
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }

// DPP move of a double without an old value (bound_ctrl, full masks): each half is one v_mov_b32_dpp that reads the source
// register itself, with no v_mov_b32 copy in front of it.  Only for controls under which every lane has a source lane
// (row_ror here).
template <int CTRL>
__device__ __forceinline__ double dpp_src64(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true));
}

// Sum FOUR per-lane doubles over the 64 lanes in one pass ("transpose" reduction):
// returns, in every lane L, the wave total of quantity (L & 3) where the quantities are
// ordered (q0, q1, q2, q3).  7 double adds instead of 24, no LDS traffic.
__device__ __forceinline__ double wave_sum4(double q0, double q1, double q2, double q3, int lane) {
    // step 1 (partner lane^1): even lanes keep (q0,q2), odd lanes keep (q1,q3)
    const bool odd = lane & 1;
    const double k0 = odd ? q1 : q0, k1 = odd ? q3 : q2;      // kept
    const double s0 = odd ? q0 : q1, s1 = odd ? q2 : q3;      // what the partner keeps
    const double a0 = k0 + dpp_mov64<0xB1>(s0);               // quad_perm [1,0,3,2]
    const double a1 = k1 + dpp_mov64<0xB1>(s1);
    // step 2 (partner lane^2): bit1 == 0 keeps the first, bit1 == 1 keeps the second
    const bool b1 = lane & 2;
    const double kk = b1 ? a1 : a0, ss = b1 ? a0 : a1;
    double v = kk + dpp_mov64<0x4E>(ss);                      // quad_perm [2,3,0,1]
    // now lane L holds quantity (L&3) summed over its quad; rotate-add within the 16-lane row
    v = v + dpp_src64<0x124>(v);                              // row_ror:4
    v = v + dpp_src64<0x128>(v);                              // row_ror:8
    // across the four rows: swap-add with v_permlane16_swap / v_permlane32_swap
    {
        unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        unsigned lo2 = lo, hi2 = hi;
        asm("" : "+v"(lo2), "+v"(hi2));
        const v2u rl = __builtin_amdgcn_permlane16_swap(lo, lo2, false, false);
        const v2u rh = __builtin_amdgcn_permlane16_swap(hi, hi2, false, false);
        const unsigned rlx = rl.x, rly = rl.y, rhx = rh.x, rhy = rh.y;
        v = __hiloint2double((int)rhx, (int)rlx) + __hiloint2double((int)rhy, (int)rly);
    }
    {
        unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        unsigned lo2 = lo, hi2 = hi;
        asm("" : "+v"(lo2), "+v"(hi2));
        const v2u rl = __builtin_amdgcn_permlane32_swap(lo, lo2, false, false);
        const v2u rh = __builtin_amdgcn_permlane32_swap(hi, hi2, false, false);
        const unsigned rlx = rl.x, rly = rl.y, rhx = rh.x, rhy = rh.y;
        v = __hiloint2double((int)rhx, (int)rlx) + __hiloint2double((int)rhy, (int)rly);
    }
    return v;
}

// DPP source operand without an old value (bound_ctrl, full masks): hipcc folds it into the instruction that consumes
// it (v_xor_b32_dpp, v_or_b32_dpp) instead of emitting a copy and a v_mov_b32_dpp in front of it.  Only for controls
// under which every lane has a source lane (quad_perm).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_src(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ float max3_f32(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// Index of the FIRST maximum of a 21-column float32 row at LDS byte address `row`: what
//     b = v[0]; i = 0; for (j = 1; j < 21; j++) if (v[j] > b) { b = v[j]; i = j; }
// returns, in 30 vector instructions instead of 60.  The row maximum m comes from ten v_max3_f32 over seven groups
// of three columns; a descending scan with inline-constant group numbers finds the first group whose maximum equals m,
// that group's first two columns are read again and two more compares place m inside it.
// Same result as the loop for every value arithmetic can produce: v_cmp_eq_f32 and `>` agree on +-0 (neither is
// greater, both are equal), v_max3_f32 skips a quiet NaN exactly as `>` does in columns 1-20, and a NaN in column 0
// (nothing is greater than it: the loop answers 0) is tested for at the end.  (A SIGNALLING NaN, which no arithmetic
// produces, would make v_max3_f32 return NaN under the kernel's IEEE mode.)
__device__ __forceinline__ uint32_t argmax21_first(unsigned row) {
    float g[7];
#pragma unroll
    for (int k = 0; k < 7; k++)
        g[k] = max3_f32(lds_load<float>(row + 12u * k), lds_load<float>(row + 12u * k + 4u), lds_load<float>(row + 12u * k + 8u));
    const float m = max3_f32(max3_f32(g[0], g[1], g[2]), max3_f32(g[3], g[4], g[5]), g[6]);
    uint32_t c3 = 18u;                                       // first column of the first group that holds m
#pragma unroll
    for (int k = 5; k >= 0; k--) c3 = (g[k] == m) ? (uint32_t)(3 * k) : c3;
    const unsigned ad = row + 4u * c3;
    const float va = lds_load<float>(ad), vb = lds_load<float>(ad + 4u);
    uint32_t pos = (vb == m) ? 1u : 2u;
    pos = (va == m) ? 0u : pos;
    const float v0 = lds_load<float>(row);
    return (v0 != v0) ? 0u : c3 + pos;
}

__device__ __forceinline__ uint32_t readlane_u(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// v = lane `lane` of `old` replaced by the (uniform) value `val`: one v_writelane_b32 with the
// lane select in M0 (two different SGPR operands would break the gfx9 constant-bus limit)
__device__ __forceinline__ uint32_t writelane_u(uint32_t old, uint32_t val, int lane) {
    asm("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(old) : "s"(val), "s"(lane));
    return old;
}

// lo16(x) + hi16(x) in one VALU instruction (sub-dword operand selects)
__device__ __forceinline__ uint32_t halves_sum(uint32_t x) {
    uint32_t y;
    asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "=v"(y) : "v"(x));
    return y;
}

// Four steps of the play chain for one-register row tables: s <- nsr_j[s & 63] for j = 0..3, and the
// four states the steps were played in recorded TWO PER LANE (lane t0: s_t0 | s_t0+1 << 16, lane t0+2:
// s_t0+2 | s_t0+3 << 16; the caller unpacks lane-parallel) -- 6 vector instructions per group instead of 8.
// Hand-placed wait states (hipcc does not look inside asm): a v_readlane whose lane select was written by
// a VALU (the previous v_readlane) needs 4 wait states; the s_pack and the v_writelane (lane number as an
// immediate: the step numbers are compile-time constants) fill them where they can, s_nop pads the rest.
template <int T0>
__device__ __forceinline__ void chain_group(uint32_t& sq, int& s, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3) {
    int s1, s2, s3, s4, pk;
    asm volatile(
        "s_nop 3\n\t"
        "v_readlane_b32 %1, %7, %6\n\t"
        "s_pack_ll_b32_b16 %5, %6, %1\n\t"
        "v_writelane_b32 %0, %5, %11\n\t"
        "s_nop 1\n\t"
        "v_readlane_b32 %2, %8, %1\n\t"
        "s_nop 3\n\t"
        "v_readlane_b32 %3, %9, %2\n\t"
        "s_pack_ll_b32_b16 %5, %2, %3\n\t"
        "v_writelane_b32 %0, %5, %12\n\t"
        "s_nop 1\n\t"
        "v_readlane_b32 %4, %10, %3"
        : "+v"(sq), "=&s"(s1), "=&s"(s2), "=&s"(s3), "=&s"(s4), "=&s"(pk)
        : "s"(s), "v"(n0), "v"(n1), "v"(n2), "v"(n3), "n"(T0), "n"(T0 + 2)
        : "scc");
    s = s4;
}

// The same for four steps in which nobody explores: with G = "next row of a greedy step" composed with itself
// (g1 = G, g2 = G.G, g3 = G.G.G, g4 = G^4, built once per episode) the four reads all use the group's entry
// state, so only the first waits for it.
template <int T0>
__device__ __forceinline__ void chain_group_greedy(uint32_t& sq, int& s, uint32_t g1, uint32_t g2, uint32_t g3, uint32_t g4) {
    int s1, s2, s3, s4, pk;
    asm volatile(
        "s_nop 3\n\t"
        "v_readlane_b32 %1, %7, %6\n\t"
        "v_readlane_b32 %2, %8, %6\n\t"
        "v_readlane_b32 %3, %9, %6\n\t"
        "v_readlane_b32 %4, %10, %6\n\t"
        "s_pack_ll_b32_b16 %5, %6, %1\n\t"
        "v_writelane_b32 %0, %5, %11\n\t"
        "s_pack_ll_b32_b16 %5, %2, %3\n\t"
        "v_writelane_b32 %0, %5, %12"
        : "+v"(sq), "=&s"(s1), "=&s"(s2), "=&s"(s3), "=&s"(s4), "=&s"(pk)
        : "s"(s), "v"(g1), "v"(g2), "v"(g3), "v"(g4), "n"(T0), "n"(T0 + 2)
        : "scc");
    s = s4;
}

template <bool ON> struct GreedyTables {            // (nothing in the variants that do not use them)
    __device__ __forceinline__ void build(unsigned) {}
    template <int T0> __device__ __forceinline__ void chain(uint32_t&, int&) const {}
};
template <> struct GreedyTables<true> {
    uint32_t g1, g2, g3, g4;
    __device__ __forceinline__ void build(unsigned lut_addr) {
        g1 = (uint32_t)lds_load<unsigned short>(lut_addr);
        g2 = bperm((g1 & 63u) << 2, g1);
        g3 = bperm((g2 & 63u) << 2, g1);
        g4 = bperm((g2 & 63u) << 2, g2);
    }
    template <int T0> __device__ __forceinline__ void chain(uint32_t& sq, int& s) const { chain_group_greedy<T0>(sq, s, g1, g2, g3, g4); }
};

// value of a lane-indexed-by-row register pair at (uniform) row s
template <int NRSEG>
__device__ __forceinline__ uint32_t read_row(const uint32_t (&r)[NRSEG], int s) {
    uint32_t v = readlane_u(r[0], s & 63);
    if (NRSEG > 1) {
        const uint32_t h = readlane_u(r[NRSEG - 1], s & 63);
        if (s >= 64) v = h;
    }
    return v;
}
// per-lane gather from a lane-indexed-by-row register pair (row differs per lane)
template <int NRSEG>
__device__ __forceinline__ uint32_t gather_row(const uint32_t (&r)[NRSEG], uint32_t row) {
    uint32_t v = bperm((row & 63u) << 2, r[0]);
    if (NRSEG > 1) {
        const uint32_t h = bperm((row & 63u) << 2, r[NRSEG - 1]);
        if (row >= 64u) v = h;
    }
    return v;
}

// ---- table-type dependent pieces of train_net's arithmetic (thrl_device.h td_value) ------------
// Operands of one 32-transition block in "step layout": lane 32h + t = agent h, transition t.
// float : c1 = fma(alpha, reward, (1-alpha)*old_value) -- everything of the target that does not
//         depend on the live next_max; the pass then executes ONE fma (thrl_device.h, float32 form).
// double: the reference's four separately rounded operations need reward and (1-alpha)*old_value.
template <typename QT> struct BlockOps;
template <> struct BlockOps<float> {
    unsigned c1;
    __device__ __forceinline__ void permute(unsigned sel) { c1 = bperm(sel, c1); }
    __device__ __forceinline__ void keep() const { asm volatile("" :: "v"(c1)); }
    __device__ __forceinline__ float value(float nm, float alpha_gamma, float, float) const {
        return __fmaf_rn(alpha_gamma, nm, __builtin_bit_cast(float, c1));
    }
};
template <> struct BlockOps<double> {
    unsigned r_lo, r_hi, t4_lo, t4_hi;
    __device__ __forceinline__ void keep() const { asm volatile("" :: "v"(r_lo), "v"(r_hi), "v"(t4_lo), "v"(t4_hi)); }
    __device__ __forceinline__ void permute(unsigned sel) {
        r_lo = bperm(sel, r_lo); r_hi = bperm(sel, r_hi); t4_lo = bperm(sel, t4_lo); t4_hi = bperm(sel, t4_hi);
    }
    __device__ __forceinline__ double value(double nm, double, double alpha, double gamma) const {
        const double re = __hiloint2double((int)r_hi, (int)r_lo), t4 = __hiloint2double((int)t4_hi, (int)t4_lo);
        const double t2 = __dadd_rn(re, __dmul_rn(gamma, nm));                 // agents.py:73
        return __dadd_rn(t4, __dmul_rn(alpha, t2));                           // agents.py:72,74
    }
};
// (1-alpha)*old_value of both agents for the 64 transitions of a segment, halves packed per 32
template <typename QT> struct Snapshot;
template <> struct Snapshot<float> {
    v2u t4;
    __device__ __forceinline__ void set(float oma0, float ov0, float oma1, float ov1) {
        t4 = pack_halves(__builtin_bit_cast(unsigned, __fmul_rn(oma0, ov0)), __builtin_bit_cast(unsigned, __fmul_rn(oma1, ov1)));
    }
};
template <> struct Snapshot<double> {
    v2u lo, hi;
    __device__ __forceinline__ void set(double oma0, double ov0, double oma1, double ov1) {
        const double x0 = __dmul_rn(oma0, ov0), x1 = __dmul_rn(oma1, ov1);
        lo = pack_halves((unsigned)__double2loint(x0), (unsigned)__double2loint(x1));
        hi = pack_halves((unsigned)__double2hiint(x0), (unsigned)__double2hiint(x1));
    }
};
__device__ __forceinline__ BlockOps<float> make_ops(const Snapshot<float>& s, int k, double r0d, double r1d, float alpha_h) {
    const v2u req = pack_halves(__builtin_bit_cast(unsigned, (float)r0d), __builtin_bit_cast(unsigned, (float)r1d));
    BlockOps<float> o;
    o.c1 = __builtin_bit_cast(unsigned, __fmaf_rn(alpha_h, __builtin_bit_cast(float, k ? req.y : req.x),
                                                  __builtin_bit_cast(float, k ? s.t4.y : s.t4.x)));
    return o;
}
__device__ __forceinline__ BlockOps<double> make_ops(const Snapshot<double>& s, int k, double r0d, double r1d, double) {
    const v2u rl = pack_halves((unsigned)__double2loint(r0d), (unsigned)__double2loint(r1d));
    const v2u rh = pack_halves((unsigned)__double2hiint(r0d), (unsigned)__double2hiint(r1d));
    BlockOps<double> o;
    o.r_lo = k ? rl.y : rl.x; o.r_hi = k ? rh.y : rh.x;
    o.t4_lo = k ? s.lo.y : s.lo.x; o.t4_hi = k ? s.hi.y : s.hi.x;
    return o;
}
// per-agent hyper-parameters in the table's arithmetic type
template <typename QT> struct HP;
template <> struct HP<float> {
    static __device__ __forceinline__ float gamma(const AgentParams& p) { return p.gamma_f; }
    static __device__ __forceinline__ float alpha(const AgentParams& p) { return p.alpha_f; }
    static __device__ __forceinline__ float one_minus_alpha(const AgentParams& p) { return p.one_minus_alpha_f; }
    static __device__ __forceinline__ float from_double(double x) { return (float)x; }
    static __device__ __forceinline__ float product(float a, float g) { return __fmul_rn(a, g); }
};
template <> struct HP<double> {
    static __device__ __forceinline__ double gamma(const AgentParams& p) { return p.gamma; }
    static __device__ __forceinline__ double alpha(const AgentParams& p) { return p.alpha; }
    static __device__ __forceinline__ double one_minus_alpha(const AgentParams& p) { return p.one_minus_alpha; }
    static __device__ __forceinline__ double from_double(double x) { return x; }
    static __device__ __forceinline__ double product(double, double) { return 0.0; }    // unused in float64 mode
};

// One 32-transition block of train_net's loop (agents.py:68-76), four transitions per pass.
// RDN = row reads per lane: 2 (A = 2), 3 (A <= 24) or 4; a lane reads RDN CONSECUTIVE columns of its
// transition's next-state row (one address: the loads differ by an immediate offset).
//   P        (step layout, lane 4g of the segment): the four next-state rows of group g, 7 bits each,
//            | cut bits << 28 (bit j-1: a new pass starts before transition j of the group)
//            | bit 31: the four transitions are IDENTICAL and stay in their row (a converged game sits in a
//              fixed point: same state, same greedy actions, same reward, step after step).  Serially that
//              is four dependent (row max, TD value) pairs on one cell; here the row is read once, split
//              into "the cell" and "max of the rest", and the four pairs run in registers: one store.
//   ops, wo  operands / LDS store address of transition 4*(lane&7) + ((lane>>3)&3) ("exec layout")
//   key      (exec layout) 4 * (the transition's group) + the number of the pass it is stored in, or kKeyNone
// GI >= 0: the group number as a compile-time constant (the unrolled copies), else gi_rt.
template <typename QT, int RDN, bool FIXED_POINTS, bool PER2, int GI>
__device__ __forceinline__ void replay_group(int gi_rt, uint32_t P, int lane_base, int nsub, const BlockOps<QT>& ops, unsigned wo,
                                             unsigned key, unsigned rd_base, unsigned row_shift, unsigned my_step,
                                             unsigned row_bytes, QT alpha_gamma, QT alpha, QT gamma, bool upper_half,
                                             int block_step0, int replay_from) {
    const int gi = GI >= 0 ? GI : gi_rt;
    // transitions that had already dropped out of the deque when the buffer trained are skipped
    const int first = replay_from - (block_step0 + gi * 4);      // <= 0: the whole group trains
    if (first >= 4) return;
    const uint32_t sP = readlane_u(P, lane_base + gi * 4);
    const int nv = min(4, nsub - gi * 4);
    unsigned ad0;                                           // row * row_bytes + this lane's first column: one v_mad_u32_u24
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(ad0) : "v"((sP >> row_shift) & 0x7Fu), "s"(row_bytes), "v"(rd_base));
    unsigned ad[RDN];                                       // this lane's columns of its transition's next-state row
#pragma unroll
    for (int i = 0; i < RDN; i++) ad[i] = ad0 + (unsigned)(i * sizeof(QT));
    if (FIXED_POINTS && PER2 && (sP >> 31) && nv == 4 && first <= 0 && !(kAblate & 256) && (sP & 0x7Fu) != ((sP >> 7) & 0x7Fu)) {
        // PERIOD-2 CYCLE (A, B, A, B): A is played in row sA and leads to row sB, B leads back.  Serially that is
        // four dependent (row max, TD value) pairs: each transition reads the row its predecessor just wrote.
        // Here groups 0/2 (the A's) read row sB once and split it into "the cell B writes" and the rest, groups
        // 1/3 do the same for row sA and A's cell, and the four values run in registers, each handed to the
        // neighbouring 8-lane group by one DPP rotate: y0 = A(max row sB), y1 = B(max(rest sA, y0)),
        // y2 = A(max(rest sB, y1)), y3 = B(max(rest sA, y2)); the cells end as y2 / y3.
        // exec layout: transition 4*gi + i sits in lanes 8*i + gi / 32 + 8*i + gi
        const unsigned ca0 = readlane_u(wo, gi), ca1 = readlane_u(wo, 32 + gi);
        const unsigned cb0 = readlane_u(wo, 8 + gi), cb1 = readlane_u(wo, 40 + gi);
        const bool odd = (my_step & 1u) != 0u;                  // my_step & 3 = this lane's 8-lane group
        const unsigned cell = odd ? (upper_half ? ca1 : ca0) : (upper_half ? cb1 : cb0);
        QT rest = -(QT)INFINITY, m = -(QT)INFINITY;
#pragma unroll
        for (int i = 0; i < RDN; i++) {
            const QT e = lds_load<QT>(ad[i]);
            m = max_of(m, e);
            rest = max_of(rest, ad[i] == cell ? -(QT)INFINITY : e);
        }
        rest = group8_allmax(rest);
        m = group8_allmax(m);
        const QT y0 = ops.value(m, alpha_gamma, alpha, gamma);
        const QT y1 = ops.value(max_of(rest, dpp_ror8(y0)), alpha_gamma, alpha, gamma);
        const QT y2 = ops.value(max_of(rest, dpp_ror8(y1)), alpha_gamma, alpha, gamma);
        const QT y3 = ops.value(max_of(rest, dpp_ror8(y2)), alpha_gamma, alpha, gamma);
        store_where(__ballot((unsigned)(my_step - (unsigned)(gi * 4 + 2)) < 2u), wo, odd ? y3 : y2);
        __builtin_amdgcn_wave_barrier();
        return;
    }
    if (FIXED_POINTS && (sP >> 31) && nv == 4 && first <= 0 && !(kAblate & 256)) {
        // the rewritten cell, per agent: lanes gi / 32+gi hold transition 4*gi's store address
        const unsigned c0 = readlane_u(wo, gi), c1 = readlane_u(wo, 32 + gi);
        const unsigned cell = upper_half ? c1 : c0;
        QT rest = -(QT)INFINITY, cur = -(QT)INFINITY;
#pragma unroll
        for (int i = 0; i < RDN; i++) {
            const QT e = lds_load<QT>(ad[i]);
            rest = max_of(rest, ad[i] == cell ? -(QT)INFINITY : e);
            cur = max_of(cur, ad[i] == cell ? e : -(QT)INFINITY);
        }
        rest = group8_allmax(rest);
        cur = group8_allmax(cur);
#pragma unroll
        for (int k = 0; k < 4; k++) cur = ops.value(max_of(rest, cur), alpha_gamma, alpha, gamma);
        if (my_step == (unsigned)(gi * 4 + 3)) lds_store<QT>(wo, cur);
        __builtin_amdgcn_wave_barrier();
        return;
    }
    // The ordinary passes.  Pass k holds the transitions between the k-th and the (k+1)-th cut of the group, exactly
    // the serial loop's [lo, hi) ranges in the same order; phase (d2) has numbered them per lane (the key), has kept
    // only the cuts between two transitions that train, and has given the others no key.  So pass 0 runs
    // unconditionally, one scalar test of the cut bits finds the groups that need more, and a pass is row reads,
    // row maximum, TD value and the store by the lanes whose key matches: no range, no ballot, no EXEC bookkeeping.
    auto td_value = [&]() -> QT {
        QT m = lds_load<QT>(ad[0]);
#pragma unroll
        for (int i = 1; i < RDN; i++) m = max_of(m, lds_load<QT>(ad[i]));
        m = group8_allmax(m);
        return ops.value(m, alpha_gamma, alpha, gamma);
    };
    store_key<(GI >= 0 ? 4 * GI : -1)>(key, (unsigned)(gi * 4), wo, td_value());
    __builtin_amdgcn_wave_barrier();
    if (sP & 0x70000000u) {
        unsigned k = (unsigned)(gi * 4 + 1);
        const unsigned last = (unsigned)(gi * 4) + (unsigned)__builtin_popcount((sP >> 28) & 7u);
        do {
            store_key<-1>(key, k, wo, td_value());
            __builtin_amdgcn_wave_barrier();
        } while (++k <= last);
    }
}
// the block's groups GI... as straight-line code; BOUNDED: stop at the first group behind the block's end
template <typename QT, int RDN, bool FIXED_POINTS, bool PER2, bool BOUNDED, int... GI>
__device__ __forceinline__ void replay_groups(std::integer_sequence<int, GI...>, uint32_t P, int lane_base, int nsub, const BlockOps<QT>& ops,
                                              unsigned wo, unsigned key, unsigned rd_base, unsigned row_shift, unsigned my_step,
                                              unsigned row_bytes, QT alpha_gamma, QT alpha, QT gamma, bool upper_half,
                                              int block_step0, int replay_from) {
    (void)(((!BOUNDED || GI * 4 < nsub) &&
            (replay_group<QT, RDN, FIXED_POINTS, PER2, GI>(GI, P, lane_base, nsub, ops, wo, key, rd_base, row_shift, my_step, row_bytes,
                                                           alpha_gamma, alpha, gamma, upper_half, block_step0, replay_from), true)) && ...);
}
// UNROLL: the block's 8 groups as straight-line code (group numbers become immediates, no loop control):
// every variant with <= 128 steps per cycle except float64 + noise (hipcc 7.2 fails on that one: "illegal VGPR to SGPR copy").
//   wo_key   (exec layout) LDS store address of the lane's transition | its replay key << kKeyShift
template <typename QT, int RDN, bool FIXED_POINTS, bool UNROLL, bool PER2>
__device__ __forceinline__ void replay_block(uint32_t P, int lane_base, int nsub, const BlockOps<QT>& ops, unsigned wo_key,
                                             unsigned rd_base, unsigned row_shift, unsigned my_step,
                                             unsigned row_bytes, QT alpha_gamma, QT alpha, QT gamma, bool upper_half,
                                             int block_step0, int replay_from) {
    if (kAblate & 1) { ops.keep(); asm volatile("" :: "v"(wo_key), "v"(P)); return; }
    const unsigned key = wo_key >> kKeyShift, wo = wo_key & ((1u << kKeyShift) - 1u);
    if (UNROLL) {
        if (nsub == 32) {
            // a full block (three of the four blocks of a 100-step episode): every "is this group
            // inside the block" test folds away
            replay_groups<QT, RDN, FIXED_POINTS, PER2, false>(std::make_integer_sequence<int, 8>{}, P, lane_base, 32, ops, wo, key, rd_base,
                                                              row_shift, my_step, row_bytes, alpha_gamma, alpha, gamma, upper_half,
                                                              block_step0, replay_from);
            return;
        }
        replay_groups<QT, RDN, FIXED_POINTS, PER2, true>(std::make_integer_sequence<int, 8>{}, P, lane_base, nsub, ops, wo, key, rd_base,
                                                         row_shift, my_step, row_bytes, alpha_gamma, alpha, gamma, upper_half,
                                                         block_step0, replay_from);
    } else {
        for (int gi = 0; gi * 4 < nsub; gi++)
            replay_group<QT, RDN, FIXED_POINTS, PER2, -1>(gi, P, lane_base, nsub, ops, wo, key, rd_base, row_shift, my_step, row_bytes,
                                                          alpha_gamma, alpha, gamma, upper_half, block_step0, replay_from);
    }
}

// A segment whose transitions repeat with period P (P different rows; transition j of the cycle is played in row
// s_j, leads to row s_(j+1) and rewrites cell c_j of row s_j): train_net's serial loop (agents.py:68-76) as a
// recurrence in registers.  cur[j] = live value of c_j, rest[j] = max of row s_j without c_j (the other cells of
// the row do not change during the segment), so transition t = j (mod P) is
//     cur[j] <- TD value(max(rest[j+1], cur[j+1]))        -- the same arithmetic, in the same order, as the passes.
// ops0 / woq_x are in step layout (lane 32h + t = agent h, transition t < 32); W[j] = transition word of step j.
template <typename QT, int P>
__device__ __forceinline__ void cyclic_segment(const BlockOps<QT>& ops0, unsigned woq_x, const uint32_t (&W)[4], int nseg, int lane,
                                               unsigned tabh, int A, unsigned row_bytes, QT alpha_gamma, QT alpha, QT gamma) {
    BlockOps<QT> ops[P];
    unsigned cell[P];
    QT rest[P], cur[P];
    const unsigned colb = (unsigned)min(lane & 31, A - 1) * (unsigned)sizeof(QT);
#pragma unroll
    for (int j = 0; j < P; j++) {
        const unsigned sel = (unsigned)((lane & 32) + j) << 2;
        ops[j] = ops0;
        ops[j].permute(sel);
        cell[j] = bperm(sel, woq_x);
        const unsigned ad = tabh + ((W[j] >> 16) & 0xFFu) * row_bytes + colb;
        const QT v = lds_load<QT>(ad);
        cur[j] = lds_load<QT>(cell[j]);
        rest[j] = half32_allmax(ad == cell[j] ? -(QT)INFINITY : v);
    }
    int t = 0;
    for (; t + P <= nseg; t += P) {
#pragma unroll
        for (int j = 0; j < P; j++) cur[j] = ops[j].value(max_of(rest[(j + 1) % P], cur[(j + 1) % P]), alpha_gamma, alpha, gamma);
    }
#pragma unroll
    for (int j = 0; j < P; j++)
        if (t + j < nseg) cur[j] = ops[j].value(max_of(rest[(j + 1) % P], cur[(j + 1) % P]), alpha_gamma, alpha, gamma);
    if ((lane & 31) == 0) {
#pragma unroll
        for (int j = 0; j < P; j++) lds_store<QT>(cell[j], cur[j]);
    }
}

// ---- play phase of the AFFINE variants: one segment (up to 64 steps) of an episode ----------------------------------
// On an affine payoff grid (thrl_api.hip plan_wave) the row after an action pair is  c - m0*a0 - m1*a1  (local rows,
// float32 and float64 encodes alike), so "the next row if step t were played in row r" is
//     nsr_t[r] = kb_t - (g0[r] & m0b_t) - (g1[r] & m1b_t)
// with, per row r,  g_i[r] = m_i * (greedy action of agent i in row r)  and, per step t,
//     m_ib_t = agent i explores in step t ? 0 : 0xFF,     kb_t = c - (explore0 ? m0*c0 : 0) - (explore1 ? m1*c1 : 0).
// All of these are bytes (<= c <= 61), so the tables of FOUR consecutive steps are one dword per row: the step-side bytes of
// steps 4g..4g+3 sit in three dwords (M0q, M1q, Kq) of the wave's 256-byte LDS area, 16 bytes per group, written once per
// segment with byte stores (lane = step); a group's table is then
//     Tq = Kq - (G0q & M0q) - (G1q & M1q)                 (lane = row; G_iq = g_i[r] in all four bytes)
// after ONE uniform-address LDS read: two ands and two subtractions on VGPRs, no gather from the payoff LUT.
// No borrow crosses a byte: in every byte  kb - (g0 & m0b)  and  kb - (g0 & m0b) - (g1 & m1b)  are at least the row that
// the action pair (explore ? choice : greedy) leads to, which the plan guarantees to be >= 0 for every pair -- whatever
// the neighbouring bytes hold.  (hipcc reassociates to Kq - ((G0q & M0q) + (G1q & M1q)): the same value mod 2^32, and the
// sum is at most kb <= c in every byte, so it does not carry either.)  tests/test_wave_affine_host.py enumerates this.
// Chain: byte j of Tq, read at the lane of the current row, is the row after step 4g+j; v_readlane takes the low six bits
// of its lane select.  The four rows the steps were played in are recorded as the bytes of ONE word in lane 4g
// (assembled on the scalar unit) and unpacked lane-parallel after the chain.
// s: play row | train row << 8 on entry (they differ only in a launch's first step from a continuous price) and on exit;
// returns seq: lane t = the state step t was played in, in the same 16-bit form.
__device__ __forceinline__ uint32_t pack16(uint32_t lo, uint32_t hi) {      // lo | hi << 16 of two values < 2^16: one s_pack
    typedef unsigned short v2h __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, v2h{(unsigned short)lo, (unsigned short)hi});
}
// lane L (an immediate) of `old` replaced by the uniform value `val`
template <int L>
__device__ __forceinline__ uint32_t writelane_imm(uint32_t old, uint32_t val) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "n"(L));
    return old;
}
template <int T0>
__device__ __forceinline__ void chain_group_affine(uint32_t& sq, uint32_t& sc, uint32_t Tq) {
    const uint32_t s1 = readlane_u(Tq, (int)sc) & 0xFFu;
    const uint32_t s2 = (readlane_u(Tq, (int)s1) >> 8) & 0xFFu;
    const uint32_t s3 = (readlane_u(Tq, (int)s2) >> 16) & 0xFFu;
    const uint32_t s4 = readlane_u(Tq, (int)s3) >> 24;
    const uint32_t w = pack16(sc, s2) | (pack16(s1, s3) << 8);                // s0 | s1 << 8 | s2 << 16 | s3 << 24
    sq = writelane_imm<T0>(sq, w);
    sc = s4;
}
__device__ __forceinline__ uint32_t play_affine(int seg, int n, int lane, uint32_t rw, uint32_t G0q, uint32_t G1q, unsigned mk_addr,
                                                int c, int m0, int m1, int& s) {
    const int s_entry = __builtin_amdgcn_readfirstlane(s);       // ("s" operands must be provably uniform)
    {   // step side (lane = step): three bytes per step
        const uint32_t kb = (uint32_t)c - ((rw & 1u) ? ((rw >> 8) & 0xFFu) * (uint32_t)m0 : 0u)
                                        - ((rw & 2u) ? ((rw >> 16) & 0xFFu) * (uint32_t)m1 : 0u);
        const unsigned ad = mk_addr + 16u * (unsigned)(lane >> 2) + (unsigned)(lane & 3);
        lds_store<unsigned char>(ad, (rw & 1u) ? (unsigned char)0 : (unsigned char)0xFF);
        lds_store<unsigned char>(ad + 4u, (rw & 2u) ? (unsigned char)0 : (unsigned char)0xFF);
        lds_store<unsigned char>(ad + 8u, (unsigned char)kb);
        __builtin_amdgcn_wave_barrier();
    }
    // the area is 8-byte aligned (plan_wave): two adjacent 8-byte reads, which hipcc issues as one ds_read2_b64
    struct Q4 { v2u lo, hi; };
    auto loadq = [&](int g) {
        Q4 q;
        q.lo = lds_load<v2u>(mk_addr + 16u * (unsigned)g);
        q.hi = lds_load<v2u>(mk_addr + 16u * (unsigned)g + 8u);
        return q;
    };
    auto make = [&](const Q4& q) {
        asm volatile("" :: "v"(q.hi.y));      // (keeps the second read 8 bytes wide, so that the two merge)
        return q.hi.x - (G0q & q.lo.x) - (G1q & q.lo.y);
    };
    uint32_t sq = 0u, sq_tail = 0u;           // sq: lane 4g = the four states of full group g; sq_tail: one state per lane
    uint32_t sc = (uint32_t)s_entry & 0xFFu;     // the chain runs on the play row
    // One group's chain.  The scheduling barriers around it keep the LDS read issued in front of it and the table built
    // behind it where they are written: hipcc otherwise sinks the read to its first use and the chain waits for the LDS there.
    auto chain4 = [&](auto t0c, const int nn, const uint32_t Tq) {
        constexpr int t0 = decltype(t0c)::value;
        __builtin_amdgcn_sched_barrier(0);
        if (t0 + 4 <= nn) chain_group_affine<t0>(sq, sc, Tq);
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (t0 + j < nn) {
                    sq_tail = writelane_u(sq_tail, sc * 0x101u, t0 + j);
                    sc = (readlane_u(Tq, (int)sc) >> (8 * j)) & 0xFFu;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // Pipeline: the step bytes of group g+2 are requested before group g's chain, and the table of group g+1 is built from
    // bytes requested a whole chain earlier, right after group g's chain.  (Entering THRL_PLAYA2(G): Ta = table of group G,
    // qb = bytes of group G+1.)
    Q4 qa = loadq(0), qb = loadq(1);
    uint32_t Ta = make(qa), Tb = 0u;
#define THRL_PLAYA2(G, N_)                                                                   \
    if ((G) * 4 < (N_)) {                                                                    \
        if ((G) * 4 + 8 < (N_)) qa = loadq((G) + 2 < 15 ? (G) + 2 : 15);                     \
        chain4(std::integral_constant<int, (G) * 4>(), (N_), Ta);                            \
        if ((G) * 4 + 4 < (N_)) {                                                            \
            Tb = make(qb);                                                                   \
            if ((G) * 4 + 12 < (N_)) qb = loadq((G) + 3 < 15 ? (G) + 3 : 15);                \
            chain4(std::integral_constant<int, (G) * 4 + 4>(), (N_), Tb);                    \
            if ((G) * 4 + 8 < (N_)) Ta = make(qa);                                           \
        }                                                                                    \
    }
#define THRL_PLAYA16(N_)                                                                     \
    THRL_PLAYA2(0, N_) THRL_PLAYA2(2, N_) THRL_PLAYA2(4, N_) THRL_PLAYA2(6, N_)              \
    THRL_PLAYA2(8, N_) THRL_PLAYA2(10, N_) THRL_PLAYA2(12, N_) THRL_PLAYA2(14, N_)
    // full segments and the 36-step second segment of a 100-step episode run copies without the tests
    if (n == 64) { THRL_PLAYA16(64) } else if (n == 36) { THRL_PLAYA16(36) } else { THRL_PLAYA16(n) }
#undef THRL_PLAYA16
#undef THRL_PLAYA2
    s = (int)(sc * 0x101u);                    // after a step the play and the train row are the same
    // unpack: lane t takes byte t & 3 of its quad's first lane
    // (the s_nop: a DPP read of a VGPR that the chain's last v_writelane may just have written needs 2 wait states, and hipcc
    //  does not look inside asm statements)
    uint32_t qd;
    asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf" : "=v"(qd) : "v"(sq));
    const uint32_t un = ((qd >> (8u * (unsigned)(lane & 3))) & 0xFFu) * 0x101u;
    uint32_t out = lane < (n & ~3) ? un : sq_tail;
    // the first step of the episode carries the entry state's own train row
    if (seg == 0) out = writelane_imm<0>(out, (uint32_t)s_entry);
    return out;
}

// LDS capacity allows 20 resident waves per CU for the headline window in float32, i.e. 5 per
// SIMD: keep the register allocation at <= 96 VGPRs there (NSEG <= 2).  float64 tables are twice
// the size (11 games per CU), so the register budget is relaxed there.
// NOISE: environment noise (environments.py:28-31) handled per step (price not on the LUT);
// its larger row window leaves room for fewer waves, so the register budget is relaxed.
// SWEEP: per-game hyper-parameter arrays (thrl_buffers.sweep_*); compiled only together with NOISE
// so the headline variant carries none of that state.
// LOG: per-game log rows (thrl_buffers.game_reward_log / game_action_log).  A template flag, so the unlogged
// variants compile exactly as without the store: with a run-time null test the headline launch lost 1.8 %.
// AFFINE: closed-form play tables (WaveArgs.aff_*; plain float32 variants with one row register only): on a payoff grid
// whose next row is affine in the two action indices, phases (b, c) build the next-row tables of four steps at once by
// byte-parallel integer arithmetic instead of four gathers from the payoff LUT (play_affine below).
template <typename QT, int NSEG, int NRSEG, bool NOISE, bool SWEEP, bool CYCLE, bool GREEDY = false, bool LOG = false, bool AFFINE = false>
__global__ void __launch_bounds__(1024)
__attribute__((amdgpu_waves_per_eu(sizeof(QT) == 8 ? 3 : (NOISE ? 4 : (NSEG <= 2 ? 5 : 4)))))
k_wave_episodes(const WaveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(!AFFINE || (sizeof(QT) == 4 && !NOISE && !SWEEP && !CYCLE && !GREEDY && NRSEG == 1 && kAblate == 0),
                  "closed-form play tables: plain float32 variants with one row register");
    constexpr bool kUnrollReplay = NSEG <= 2 && !(NOISE && sizeof(QT) == 8);     // (hipcc 7.2 cannot compile the unrolled float64 noise variant)
    const int lane = threadIdx.x & 63;
    const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // A training cycle = epk episodes played against frozen tables (the replay buffer reaches min_memory
    // every epk-th episode), then ONE train_net over the transitions still in the deque.  T = transitions
    // per cycle; for the reference's example configs epk = 1 and a cycle is an episode.
    // CYCLE = false: the variant for epk == 1 with nothing dropped from the deque (min_memory <= T <= capacity),
    // compiled without any of the cycle bookkeeping.
    const int A = a.A, W = a.win_rows, Tenv = a.T, epk = CYCLE ? a.epk : 1, T = a.T * epk, lo = a.row_lo;
    const int replay_from = CYCLE ? a.replay_from : 0;
    const WaveLut L = wave_lut_layout(A);

    {   // stage the payoff LUT once per block
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.lut_ns);
        uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
        for (int k = threadIdx.x; k < (a.lut_bytes >> 2); k += blockDim.x) dst[k] = src[k];
    }
    __syncthreads();
    const unsigned lut_ns_lds = lds_addr(smem + L.ns_off);                            // u16 [A*A]: play row | train row << 8
    const double* lut_aq = reinterpret_cast<const double*>(smem + L.aq_off);
    const double* lut_sct = reinterpret_cast<const double*>(smem + L.sct_off);

    QT* tab0 = reinterpret_cast<QT*>(smem + a.lut_bytes + (size_t)wib * a.game_lds_bytes);
    QT* tab1 = tab0 + (W + 2) * A;
    const int half = lane >> 5;
    const unsigned tab0_off = lds_addr(tab0);        // absolute LDS byte addresses
    const unsigned tab1_off = lds_addr(tab1);
    // replay ("exec") layout of a 32-transition block: lane 32h + 8k + j  <->  agent h, transition 4j + k
    const int kk = (lane >> 3) & 3, jj = lane & 7;
    const unsigned perm_sel = (unsigned)((lane & 32) + 4 * jj + kk) << 2;      // bpermute source of this lane
    const unsigned my_step = (unsigned)(4 * jj + kk);
    const unsigned row_shift = (unsigned)(7 * kk);
    const unsigned row_bytes = (unsigned)A * (unsigned)sizeof(QT);
    // replay row reads: lane jj of an 8-lane group reads columns rdn*jj .. rdn*jj + rdn-1 (the last lanes
    // re-read the row's last rdn columns), rdn = 2 / 3 / 4 for A = 2 / <= 24 / <= 32
    const int rdn = A < 3 ? 2 : (A <= 24 ? 3 : 4);
    const unsigned rd_base = (half ? tab1_off : tab0_off) + (unsigned)sizeof(QT) * (unsigned)min(rdn * jj, A - rdn);
    // 256 bytes behind the wave's tables (float32, noise-free configurations: thrl_api.hip plan_wave): per-step words of a segment
    constexpr bool kLdsMK = sizeof(QT) == 4 && !NOISE && !GREEDY && NRSEG == 1 && !(kAblate & 6);
    const unsigned mk_addr = tab0_off + 2u * (unsigned)((W + 2) * A) * (unsigned)sizeof(QT);
    // float32 tables with 21 actions: per-row greedy actions by row maximum + scan (argmax21_first)
    constexpr bool kArgmax21 = sizeof(QT) == 4;
    // variants without the NOISE / GREEDY additions to the fixed-point flag: replay schedule from three hazard ballots and
    // scalar mask arithmetic (phase (d2))
    constexpr bool kMaskSched = !NOISE && !GREEDY;
    // variants that need an episode's log sums only in the launch's means (no per-game rows, one part per episode): phase
    // (f) parks the four undivided totals in the wave's `partial` region and the game's epilogue finishes all of the game's
    // episodes lane-parallel (divide, scale, round, add) -- once per lane and game instead of once per episode
    constexpr bool kParkLogs = !LOG && !CYCLE;

    const AgentParams& p0 = a.ag[0];
    const AgentParams& p1 = a.ag[1];
    const double inv_T_den = (double)Tenv;

    // lane ((e&15)*4+k): sum over this wave's games of episode-e log value k (e < 16 / e >= 16), as
    // fixed-point integers: the games a wave gets are not deterministic, integer sums do not care
    long long acc = 0, acc_hi = 0;
    const double log_scale = (lane & 2) ? a.log_scale[1] : a.log_scale[0];
    const int wave_gid = blockIdx.x * a.waves_per_block + wib;
    // kParkLogs: the wave's region partial[wave_gid][e][k] holds the current game's pending totals (slot 4 e + k, written by
    // lane 4 (e & 3) + k) until the kernel's last two stores put the sums there.  Lane L finishes slot L into acc and slot 64 + L into
    // acc_hi: the lane and the accumulator that log_into gives episode e = 16 pass + (L >> 2), quantity k = L & 3.
    auto load_parked = [&](int pass) {          // (L2-served like the transition log's read-back: the wave reads what it stored itself)
        return __hip_atomic_load(&a.partial[(size_t)wave_gid * 128 + 64 * pass + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto finish_parked = [&](long long p0w, long long p1w) {
#pragma unroll
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1 && a.n_episodes <= 16) break;
            double v = __longlong_as_double(pass ? p1w : p0w);
            if ((lane & 3) < 2) v = __ddiv_rn(v, inv_T_den);
            const long long vq = __double2ll_rn(__dmul_rn(v, log_scale));
            // a slot this game did not write holds anything (an earlier launch's sums): the ADD is masked, so it contributes nothing
            if (16 * pass + (lane >> 2) < a.n_episodes) { if (pass) acc_hi += vq; else acc += vq; }
        }
    };

    // Games are handed out dynamically (one atomic per game): waves on less crowded CUs simply take
    // more games, which measured 7-13 % faster than the static grid-stride assignment.
    // The NEXT game's id is claimed when a game starts, so the atomic's round trip is off the path.
    int g_claim = 0;
    if (lane == 0) g_claim = atomicAdd(a.next_game, 1);
    for (;;) {
        const int g = __builtin_amdgcn_readfirstlane(g_claim);
        if (g >= a.G) break;
        if (lane == 0) g_claim = atomicAdd(a.next_game, 1);
        const uint64_t gid = a.game_offset + (uint64_t)g;
        QT* __restrict__ q0 = reinterpret_cast<QT*>(a.q) + (int64_t)g * a.stride + p0.table_off;
        QT* __restrict__ q1 = reinterpret_cast<QT*>(a.q) + (int64_t)g * a.stride + p1.table_off;
        const double price0 = a.state[g];              // issued ahead of the table stream, used after it

        // ---- per-game hyper-parameters (sweeps) or the config's scalars
        QT gamma_h = half ? HP<QT>::gamma(p1) : HP<QT>::gamma(p0);
        QT alpha_h = half ? HP<QT>::alpha(p1) : HP<QT>::alpha(p0);
        QT oma0 = HP<QT>::one_minus_alpha(p0), oma1 = HP<QT>::one_minus_alpha(p1);
        if (SWEEP && a.sw_gamma) gamma_h = HP<QT>::from_double(a.sw_gamma[(size_t)half * a.G + g]);
        if (SWEEP && a.sw_alpha) {
            alpha_h = HP<QT>::from_double(a.sw_alpha[(size_t)half * a.G + g]);
            oma0 = HP<QT>::from_double(__dsub_rn(1.0, a.sw_alpha[g]));
            oma1 = HP<QT>::from_double(__dsub_rn(1.0, a.sw_alpha[(size_t)a.G + g]));
        }
        double epsg0 = 0.0, epsg1 = 0.0;               // per-game epsilon (sweep mode)
        const bool sw_eps_on = SWEEP && a.sw_eps != nullptr;
        if (sw_eps_on) { epsg0 = a.sw_eps[g]; epsg1 = a.sw_eps[(size_t)a.G + g]; }
        const QT ag_h = HP<QT>::product(alpha_h, gamma_h);   // float32: the only coefficient on the replay chain
        const double eend0 = (SWEEP && a.sw_eps_end) ? a.sw_eps_end[g] : p0.eps_end;
        const double eend1 = (SWEEP && a.sw_eps_end) ? a.sw_eps_end[(size_t)a.G + g] : p1.eps_end;
        const double estep0 = (SWEEP && a.sw_eps_step) ? a.sw_eps_step[g] : p0.eps_step;
        const double estep1 = (SWEEP && a.sw_eps_step) ? a.sw_eps_step[(size_t)a.G + g] : p1.eps_step;
        const double noise_prob_g = (SWEEP && a.sw_noise_prob) ? a.sw_noise_prob[g] : a.env.noise_prob;

        // ---- stream the table windows HBM -> LDS (contiguous, coalesced)
        {
            const QT* s0 = q0 + lo * A;
            const QT* s1 = q1 + lo * A;
            const int n = W * A;
            // 8 loads per agent in flight before the first LDS write (one HBM latency per
            // batch instead of one per 64 elements)
            for (int k0 = 0; k0 < n; k0 += 512) {
                QT v0[8], v1[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int k = min(k0 + j * 64 + lane, n - 1);
                    v0[j] = s0[k]; v1[j] = s1[k];
                }
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int k = k0 + j * 64 + lane;
                    if (k < n) { tab0[k] = v0[j]; tab1[k] = v1[j]; }
                }
            }
        }
        // ---- initial state -> local rows (window or spill)
        int sp = __builtin_amdgcn_readfirstlane(encode32(price0, p0));
        int st = __builtin_amdgcn_readfirstlane(encode64(price0, p0));
        sp = min(max(sp, 0), a.rows - 1);
        st = min(max(st, 0), a.rows - 1);
        int spill0 = -1, spill1 = -1, sp_l, st_l;
        if (sp >= lo && sp < lo + W) sp_l = sp - lo; else { spill0 = sp; sp_l = W; }
        if (st == sp) st_l = sp_l;
        else if (st >= lo && st < lo + W) st_l = st - lo;
        else { spill1 = st; st_l = W + 1; }

        {
            if (spill0 >= 0 && lane < A) {
                tab0[W * A + lane] = q0[spill0 * A + lane];
                tab1[W * A + lane] = q1[spill0 * A + lane];
            }
            if (spill1 >= 0 && lane < A) {
                tab0[(W + 1) * A + lane] = q0[spill1 * A + lane];
                tab1[(W + 1) * A + lane] = q1[spill1 * A + lane];
            }
        }
        __builtin_amdgcn_wave_barrier();

        int s = sp_l | (st_l << 8);          // current state: play row | train row << 8
        double last_price = price0;
        for (int e = 0; e < a.n_episodes; e += epk) {
            const uint32_t eg = (uint32_t)(a.first_episode + (uint64_t)e);

            // ---- (a) greedy action of every local row, lane = row (the table is frozen
            //          during play: agents.py only writes it in train_net).  AM = a0 | a1 << 8; R packs the
            //          two greedy byte offsets into the u16 payoff LUT: agent 0's (a0*A*2) in the low
            //          half, agent 1's (a1*2) in the high half.
            uint32_t AM[NRSEG], R[NRSEG];
            uint32_t G0q = 0u, G1q = 0u;   // AFFINE: the row's greedy terms m0 * i0 and m1 * i1, each in all four bytes
#pragma unroll
            for (int k = 0; k < NRSEG; k++) {
                const int row = min(lane + 64 * k, W + 1);
                const QT* r0 = tab0 + row * A;
                const QT* r1 = tab1 + row * A;
                QT b0 = r0[0], b1 = r1[0];
                uint32_t i0 = 0, i1 = 0;
                if (kAblate & 16) {
                } else if (kArgmax21 && A == 21) {
                    i0 = argmax21_first(tab0_off + (unsigned)row * 84u);
                    i1 = argmax21_first(tab1_off + (unsigned)row * 84u);
                } else if (A == 21) {
                    // the reference's example configs: constant trip count, so the column numbers are inline
                    // constants of the selects (no index register, no loop control): 7 instructions per column pair
#pragma unroll
                    for (int j = 1; j < 21; j++) {
                        const QT v0 = r0[j], v1 = r1[j];
                        if (v0 > b0) { b0 = v0; i0 = j; }
                        if (v1 > b1) { b1 = v1; i1 = j; }
                    }
                } else {
#pragma unroll 4
                    for (int j = 1; j < A; j++) {
                        const QT v0 = r0[j], v1 = r1[j];
                        if (v0 > b0) { b0 = v0; i0 = j; }
                        if (v1 > b1) { b1 = v1; i1 = j; }
                    }
                }
                if (kAblate & 16) { i0 = (uint32_t)(lane * 5) % (uint32_t)A; i1 = (uint32_t)(lane * 3) % (uint32_t)A; }
                AM[k] = i0 | (i1 << 8);
                R[k] = (i0 * (uint32_t)A * 2u) | (i1 << 17);
                if constexpr (AFFINE) {                       // m * i <= aff_c <= 61: the product stays inside each byte
                    G0q = i0 * ((uint32_t)a.aff_m0 * 0x01010101u);
                    G1q = i1 * ((uint32_t)a.aff_m1 * 0x01010101u);
                }
            }
            // "next row if a step in which NOBODY explores is played in row r": one table for the whole episode
            // (the tables are frozen during play).  A group of four such steps needs no per-step table at all --
            // late in training that is nearly every group.
            GreedyTables<GREEDY && NRSEG == 1> gt;          // + G composed with itself: rows after 2, 3, 4 greedy steps
            gt.build(halves_sum(R[0]) + lut_ns_lds);

            // ---- (b,c) play: lane-parallel Philox, then the serial state chain.
            //      seq[seg] lane t = row in which step t was played.
            uint32_t seq[NSEG], rwv[NSEG];
            unsigned explored_segs = 0u;   // GREEDY: bit seg = somebody explored in that segment (it cannot be one cycle then)
            double nav[NSEG];              // NOISE: the uniform(0.7a, a) draw of a noisy step (lane = step)
#pragma unroll
            for (int seg = 0; seg < NSEG; seg++) {
                int n = min(64, T - seg * 64);
                // opaque to the optimiser: the unrolled play loop's "is this group inside the segment" tests stay
                // scalar compares here instead of being hoisted out of the episode loop as spilled booleans
                asm volatile("" : "+s"(n));
                uint32_t rw;
                nav[seg] = 0.0;
                // this lane's step: episode ep of the cycle, step st of that episode; its epsilon
                const int tcl = min(seg * 64 + lane, T - 1);
                const int ep = epk == 1 ? 0 : tcl / Tenv;
                const uint32_t st_in_ep = (uint32_t)(tcl - ep * Tenv);
                double eps0, eps1;
                if (sw_eps_on) { eps0 = epsg0; eps1 = epsg1; }                       // (sweeps: epk == 1)
                else if (epk == 1) { eps0 = a.eps[e][0]; eps1 = a.eps[e][1]; }
                else { eps0 = a.eps[e + ep][0]; eps1 = a.eps[e + ep][1]; }            // per-lane read of the launch's table
                if (a.inj_u) {
                    // parity mode: the reference's recorded draws, [E][T][2][G] (agents.py:81-82)
                    const int tt = tcl;
                    const size_t k = (((size_t)e * Tenv + tt) * 2) * (size_t)a.G + (size_t)g;
                    const uint32_t ex0 = a.inj_u[k] < eps0 ? 1u : 0u;
                    const uint32_t ex1 = a.inj_u[k + a.G] < eps1 ? 2u : 0u;
                    const uint32_t c0 = min((uint32_t)(uint8_t)a.inj_choice[k], (uint32_t)(A - 1));
                    const uint32_t c1 = min((uint32_t)(uint8_t)a.inj_choice[k + a.G], (uint32_t)(A - 1));
                    rw = ex0 | ex1 | (c0 << 8) | (c1 << 16);
                } else if (kAblate & 8) {
                    const uint32_t h = (uint32_t)(lane * 2654435761u) ^ eg;
                    rw = (h & 3u) | (((h >> 4) % (uint32_t)A) << 8) | (((h >> 12) % (uint32_t)A) << 16);
                } else {
                    // the ten round keys are seed + r * constant: recomputed here by scalar adds (opaque seed) --
                    // hoisted out of the episode loop they were twenty spilled SGPRs, a v_readlane each per use
                    uint32_t seed_lo = (uint32_t)a.seed, seed_hi = (uint32_t)(a.seed >> 32);
                    asm volatile("" : "+s"(seed_lo), "+s"(seed_hi));
                    const uint64_t seed_here = ((uint64_t)seed_hi << 32) | seed_lo;
                    const u32x4 x = draw_lanes(seed_here, gid, eg + (uint32_t)ep, st_in_ep, 0u);
                    const uint32_t ex0 = u01_32(x.x) < eps0 ? 1u : 0u;
                    const uint32_t ex1 = u01_32(x.z) < eps1 ? 2u : 0u;
                    rw = ex0 | ex1 | (__umulhi(x.y, (uint32_t)A) << 8) | (__umulhi(x.w, (uint32_t)A) << 16);
                }
                if (NOISE) {               // environments.py:28-29, bit 2 of rw = noisy step
                    double nu, na;
                    if (a.inj_u) {
                        const size_t k = ((size_t)e * Tenv + tcl) * (size_t)a.G + (size_t)g;
                        nu = a.inj_noise_u[k]; na = a.inj_noise_a[k];
                    } else {
                        const u32x4 xn = draw(a.seed, gid, eg + (uint32_t)ep, st_in_ep, kStreamNoise);
                        nu = u01_32(xn.x);
                        na = __dadd_rn(a.env.noise_lo, __dmul_rn(__dsub_rn(a.env.a, a.env.noise_lo), u01_32(xn.y)));
                    }
                    if (nu < noise_prob_g) rw |= 4u;
                    nav[seg] = na;
                }
                rwv[seg] = rw;
                if constexpr (AFFINE) {
                    seq[seg] = play_affine(seg, n, lane, rw, G0q, G1q, mk_addr, a.aff_c, a.aff_m0, a.aff_m1, s);
                } else {
                // Per step (lane = step), what turns the rows' greedy offsets R into the LUT address of
                // "the next row if this step were played in row r":
                //   Mv keeps agent i's half of R iff agent i does NOT explore in this step,
                //   Kv = LUT base + 2 * (explore0 ? c0*A : 0) + 2 * (explore1 ? c1 : 0)
                // so address(r) = lo16(R[r] & Mv) + hi16(R[r] & Mv) + Kv: no scalar control per step.
                // (Deciding the category -- who explores -- on the scalar unit instead needs only 2 vector
                // instructions per step, but its branches cost more than the 3 it saves: measured 13 % slower.)
                const uint32_t Mv = ((rw & 1u) ? 0u : 0xFFFFu) | ((rw & 2u) ? 0u : 0xFFFF0000u);
                const uint32_t Kv = lut_ns_lds + 2u * (((rw & 1u) ? ((rw >> 8) & 0xFFu) * (uint32_t)A : 0u) +
                                                      ((rw & 2u) ? ((rw >> 16) & 0xFFu) : 0u));
                const unsigned long long noisy_steps = NOISE ? __ballot((rw & 4u) != 0u) : 0ull;   // scalar: no per-step readlane
                // bit 4g: group g (steps 4g..4g+3) has a step that needs its own table (somebody explores, the step is
                // noisy, or it lies beyond the segment's end)
                unsigned long long busy_groups = 0ull;
                if (GREEDY && __ballot((rw & 3u) != 0u && seg * 64 + lane < T) != 0ull) explored_segs |= 1u << seg;
                if (GREEDY && NRSEG == 1) {
                    busy_groups = __ballot((rw & (NOISE ? 7u : 3u)) != 0u || seg * 64 + lane >= T);
                    busy_groups |= busy_groups >> 1;
                    busy_groups |= busy_groups >> 2;
                }
                // GREEDY variants (launched once epsilon is small, thrl_wave.hip): the play loop looks at those bits,
                // two scalar instructions per group, and skips the table build of the all-greedy groups
                constexpr bool greedy_copy = GREEDY && NRSEG == 1 && !(kAblate & 6);
                // Phase 1 (off the serial chain, lane = ROW): nsr_t[r] for one step; its LDS gather does
                // not depend on the current state.
                auto build = [&](int t, uint32_t (&out)[NRSEG], bool may_be_noisy) {
                    const int tl = t;            // < 64: only groups that start below n <= 64 are built
                    if (NOISE && may_be_noisy) {
                        if ((noisy_steps >> tl) & 1ull) {
                            // noisy step: the price is not on the LUT; evaluate it for every row
                            const uint32_t w = readlane_u(rw, tl);
                            const double na = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(nav[seg]), tl),
                                                               __builtin_amdgcn_readlane(__double2loint(nav[seg]), tl));
                            const uint32_t c0 = (w >> 8) & 0xFFu, c1 = (w >> 16) & 0xFFu;
#pragma unroll
                            for (int k = 0; k < NRSEG; k++) {
                                const uint32_t a0r = (w & 1u) ? c0 : (AM[k] & 0xFFu), a1r = (w & 2u) ? c1 : (AM[k] >> 8);
                                const double Q = __dadd_rn(lut_aq[a0r], lut_aq[A + a1r]);
                                double pr = __dsub_rn(na, __dmul_rn(a.env.b, Q));
                                if (!(pr > 0.0)) pr = 0.0;
                                const int r32 = min(max(encode32_fast(pr, p0) - lo, 0), W - 1);
                                const int r64 = min(max(encode64_fast(pr, p0) - lo, 0), W - 1);
                                out[k] = (uint32_t)(r32 | (r64 << 8));
                            }
                            return;
                        }
                    }
                    if (kAblate & 4) {
#pragma unroll
                        for (int k = 0; k < NRSEG; k++) out[k] = (R[k] >> 17) + (uint32_t)(t & 3);
                        return;
                    }
                    const uint32_t sM = readlane_u(Mv, tl), sK = readlane_u(Kv, tl);
#pragma unroll
                    for (int k = 0; k < NRSEG; k++) out[k] = lds_load<unsigned short>(halves_sum(R[k] & sM) + sK);
                };
                // Phase 2 (the chain): s <- nsr_t[s], one v_readlane per step; the state each step was
                // played in is recorded in lane t of sq.
                uint32_t sq = 0, sq_tail = 0;          // sq: two states per lane (full groups); sq_tail: one per lane
                auto chain4 = [&](auto t0c, const int n, const uint32_t (&tab)[4][NRSEG], const bool all_greedy = false) {   // n: steps in the segment
                    constexpr int t0 = decltype(t0c)::value;
                    if (kAblate & 2) {
                        asm volatile("" :: "v"(tab[0][0]), "v"(tab[1][0]), "v"(tab[2][0]), "v"(tab[3][0]));
                        sq_tail = (uint32_t)min(lane, W - 1) * 0x101u;
                        return;
                    }
                    if (NRSEG == 1 && t0 + 4 <= n) {            // full group, one-register tables: hand-scheduled steps
                        s = __builtin_amdgcn_readfirstlane(s);      // "s" operands must be provably uniform
                        if (GREEDY && all_greedy) gt.template chain<t0>(sq, s);
                        else chain_group<t0>(sq, s, tab[0][0], tab[1][0], tab[2][0], tab[3][0]);
                        return;
                    }
                    s = __builtin_amdgcn_readfirstlane(s);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (t0 + j < n) {
                            sq_tail = writelane_u(sq_tail, (uint32_t)s, t0 + j);
                            s = (int)read_row<NRSEG>(tab[j], s & 0xFF);
                        }
                    }
                };
                // the tables of group g+1 are built (their gathers in flight) while group g's chain runs
                uint32_t ta[4][NRSEG], tb[4][NRSEG];
                // float32 plain variants: the two per-step words reach the lanes as VGPRs through a uniform-address LDS read
                // issued ONE GROUP AHEAD, so the table build runs in the fast issue class (all-VGPR v_and / v_add: 2.3 cycles per
                // instruction per SIMD against 4.1 with an SGPR operand, and no v_readlane: profiles/r03_ubench_issue.md)
                v2u mkr[4] = {v2u{0u, 0u}, v2u{0u, 0u}, v2u{0u, 0u}, v2u{0u, 0u}};
                // (256 bytes per wave hold 32 steps: lanes 0-31 write theirs before the first group, lanes 32-63 overwrite them
                //  when the build reaches step 28 -- every read of steps 0-31 has been issued by then and the LDS runs a wave's
                //  operations in order)
                if (kLdsMK) {
                    if (lane < 32) lds_store<v2u>(mk_addr + 8u * (unsigned)lane, v2u{Mv, Kv});
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int j = 0; j < 4; j++) mkr[j] = lds_load<v2u>(mk_addr + 8u * (unsigned)j);
                }
                auto build4 = [&](int t0, uint32_t (&tab)[4][NRSEG]) {
                    if (kLdsMK) {
                        unsigned ad[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) ad[j] = halves_sum(R[0] & mkr[j].x) + mkr[j].y;
#pragma unroll
                        for (int j = 0; j < 4; j++) tab[j][0] = lds_load<unsigned short>(ad[j]);
                        if (t0 == 28) {
                            if (lane >= 32) lds_store<v2u>(mk_addr + 8u * (unsigned)(lane - 32), v2u{Mv, Kv});
                            __builtin_amdgcn_wave_barrier();
                        }
#pragma unroll
                        for (int j = 0; j < 4; j++) mkr[j] = lds_load<v2u>(mk_addr + 8u * (unsigned)(min(t0 + 4 + j, 63) & 31));
                        return;
                    }
                    // one scalar test per group of four steps: a group without a noisy step (81 % of them at
                    // noise_prob 0.05) takes the straight-line path
                    if (NOISE && ((noisy_steps >> t0) & 0xFull)) {
#pragma unroll
                        for (int j = 0; j < 4; j++) build(t0 + j, tab[j], true);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; j++) build(t0 + j, tab[j], false);
                    }
                };
                // Fully unrolled over the segment's 16 groups of four steps (step numbers become immediates: no
                // index arithmetic or loop control per step; a group past the segment's end costs one scalar test).
#define THRL_PLAY2(G, N_)                                                                    \
                if ((G) * 4 < (N_)) {                                                        \
                    if ((G) * 4 + 4 < (N_)) build4((G) * 4 + 4, tb);                         \
                    chain4(std::integral_constant<int, (G) * 4>(), (N_), ta);                \
                    if ((G) * 4 + 4 < (N_)) {                                                \
                        if ((G) * 4 + 8 < (N_)) build4((G) * 4 + 8, ta);                     \
                        chain4(std::integral_constant<int, (G) * 4 + 4>(), (N_), tb);        \
                    }                                                                        \
                }
#define THRL_PLAY16(N_)                                                                      \
                THRL_PLAY2(0, N_) THRL_PLAY2(2, N_) THRL_PLAY2(4, N_) THRL_PLAY2(6, N_)      \
                THRL_PLAY2(8, N_) THRL_PLAY2(10, N_) THRL_PLAY2(12, N_) THRL_PLAY2(14, N_)
                // the same with the all-greedy groups skipping their table build (g0: the group the chain runs next)
#define THRL_PLAY2G(G, N_)                                                                   \
                if ((G) * 4 + 8 <= (N_) && g0 &&                                             \
                    !(busy_groups & (((G) * 4 + 8 < 64 ? 0x110ull : 0x10ull) << ((G) * 4)))) {   \
                    /* this group, the next one and the one after it are all-greedy: two chains, no build, one test */ \
                    chain4(std::integral_constant<int, (G) * 4>(), (N_), ta, true);          \
                    chain4(std::integral_constant<int, (G) * 4 + 4>(), (N_), tb, true);      \
                } else if ((G) * 4 < (N_)) {                                                 \
                    const bool g1 = !((busy_groups >> ((G) * 4 + 4)) & 1ull);                \
                    if ((G) * 4 + 4 < (N_) && !g1) build4((G) * 4 + 4, tb);                  \
                    chain4(std::integral_constant<int, (G) * 4>(), (N_), ta, g0);            \
                    if ((G) * 4 + 4 < (N_)) {                                                \
                        g0 = (G) * 4 + 8 < 64 && !((busy_groups >> (((G) * 4 + 8) & 63)) & 1ull);   \
                        if ((G) * 4 + 8 < (N_) && !g0) build4((G) * 4 + 8, ta);              \
                        chain4(std::integral_constant<int, (G) * 4 + 4>(), (N_), tb, g1);    \
                    }                                                                        \
                }
#define THRL_PLAY16G(N_)                                                                         \
                THRL_PLAY2G(0, N_) THRL_PLAY2G(2, N_) THRL_PLAY2G(4, N_) THRL_PLAY2G(6, N_)      \
                THRL_PLAY2G(8, N_) THRL_PLAY2G(10, N_) THRL_PLAY2G(12, N_) THRL_PLAY2G(14, N_)
                // a full segment (the first of a 100-step episode) runs a copy without any of the tests
                if (greedy_copy) {
                    bool g0 = !(busy_groups & 1ull);
                    if (!g0) build4(0, ta);
                    if (n == 64) { THRL_PLAY16G(64) } else if (n == 36) { THRL_PLAY16G(36) } else { THRL_PLAY16G(n) }
                } else {
                    build4(0, ta);
                    // (36 = the second segment of the reference's 100-step episodes: also without tests)
                    if (n == 64) { THRL_PLAY16(64) } else if (n == 36) { THRL_PLAY16(36) } else { THRL_PLAY16(n) }
                }
#undef THRL_PLAY16G
#undef THRL_PLAY2G
#undef THRL_PLAY16
#undef THRL_PLAY2
                {   // unpack: lanes below the last full group of the hand-scheduled path hold two states per even lane
                    const int packed_end = (NRSEG == 1 && !(kAblate & 2)) ? (n & ~3) : 0;
                    const uint32_t prev = dpp_mov32<0x111>(sq);                 // row_shr:1 -- lane t-1 (t odd: same row)
                    const uint32_t un = (lane & 1) ? (prev >> 16) : (sq & 0xFFFFu);
                    seq[seg] = lane < packed_end ? un : sq_tail;
                }
                }   // !AFFINE
            }
            const int s_end = s;

            // ---- (d1) lane-parallel (lane = step): actions, old-value snapshot
            //      (agents.py:67) for ALL steps before any TD write
            uint32_t act[NSEG];            // a0 | a1<<8 | train_row<<16 | next_row<<24
            // the cell word of a transition: off0 | off1 << 16, the byte offsets from tab0 of the u32 visit-histogram cells
            // of the two rewritten table cells, off0 = 4*(srow*A + a0), off1 = 4*((W+2)*A + srow*A + a1) <= 4*8191.  A table
            // cell's own offset is the same (float32) or twice that (float64).  One word serves the old-value snapshot, the
            // replay store address and the visit log; 0xFFFFFFFF is no cell word (the log's "not counted" marker).
            uint32_t cwv[NSEG];
            constexpr unsigned kCellScale = (unsigned)sizeof(QT) / 4u;
            Snapshot<QT> snap[NSEG];       // (1-alpha)*old_value, halves packed per 32 steps
#pragma unroll
            for (int seg = 0; seg < NSEG; seg++) {
                const int tt = seg * 64 + lane;
                const bool valid = tt < T;
                const uint32_t my_s = seq[seg] & 0xFFu;              // row the step was played in
                const uint32_t my_train = (seq[seg] >> 8) & 0xFFu;   // row train_net sees for that state
                const uint32_t rw = rwv[seg];
                // gather with ALL lanes active (a bpermute reads only from active lanes, and
                // the source lane here is a table row, unrelated to this lane's step), then select
                const uint32_t gam = gather_row<NRSEG>(AM, my_s);
                uint32_t a0 = (rw & 1u) ? ((rw >> 8) & 0xFFu) : (gam & 0xFFu);
                uint32_t a1 = (rw & 2u) ? ((rw >> 16) & 0xFFu) : (gam >> 8);
                // next step's word: wave_shl:1 gives lane t the value of lane t+1.  Like the gather above this needs ALL 64 lanes
                // active (a DPP lane whose source lane is inactive is not written), so it must stay outside divergent control;
                // lane 63 has no source and keeps its own word, which is never used as it is: fixed up below, replaced by s_end, or not valid
                uint32_t nxt = dpp_mov32<0x130>(seq[seg]);
                if (seg + 1 < NSEG) { if (lane == 63) nxt = readlane_u(seq[seg + 1 < NSEG ? seg + 1 : seg], 0); }
                const uint32_t ns = (tt + 1 < T) ? ((nxt >> 8) & 0xFFu) : ((uint32_t)s_end >> 8);
                uint32_t srow = my_train;
                if (!valid) { a0 = 0; a1 = 0; srow = 0; }
                const uint32_t rowc = __umul24(srow, (uint32_t)A);
                const uint32_t cw = ((rowc + a0) | ((rowc + a1 + (uint32_t)((W + 2) * A)) << 16)) << 2;
                cwv[seg] = cw;
                snap[seg].set(oma0, lds_load<QT>(tab0_off + (cw & 0xFFFFu) * kCellScale),
                              oma1, lds_load<QT>(tab0_off + (cw >> 16) * kCellScale));
                act[seg] = a0 | (a1 << 8) | (srow << 16) | (ns << 24);
            }
            __builtin_amdgcn_wave_barrier();

            double lr0 = 0.0, lr1 = 0.0, la0 = 0.0, la1 = 0.0;
            // first: this call carries the first part of episode epi (a CYCLE segment holds parts of several episodes)
            auto log_into = [&](int epi, double q0, double q1, double q2, double q3, bool first) {
                double v = (kAblate & 64) ? q0 + q1 + q2 + q3 : wave_sum4(q0, q1, q2, q3, lane);
                if ((lane & 3) < 2) v = __ddiv_rn(v, inv_T_den);
                if constexpr (LOG) {   // per-game rows [epi][agent][g] of this launch: lanes 0-3 hold this game's four totals (of this part)
                    double *grl, *gal;
                    game_log_ptrs<WaveArgs>(grl, gal);
                    if (grl && lane < 2) {
                        double* p = grl + ((size_t)epi * 2 + lane) * a.G + g;
                        *p = first ? v : *p + v;
                    }
                    if (gal && (lane >> 1) == 1) {
                        double* p = gal + ((size_t)epi * 2 + (lane & 1)) * a.G + g;
                        *p = first ? v : *p + v;
                    }
                }
                const long long vq = __double2ll_rn(__dmul_rn(v, log_scale));
                if ((lane >> 2) == (epi & 15)) { if (epi < 16) acc += vq; else acc_hi += vq; }
            };
#pragma unroll
            for (int seg = 0; seg < NSEG; seg++) {
                // ---- (d2) rewards, LDS write addresses, logs, visit counters of this segment
                const int tt = seg * 64 + lane;
                const bool valid = tt < T;
                const uint32_t a0 = act[seg] & 0xFFu, a1 = (act[seg] >> 8) & 0xFFu;
                // NoisyPriceState.step (environments.py:25-39) from the staged quantities A_i = (a/b)*scaled_i:
                // three float64 operations per 64 steps instead of a gather from the L2-resident price table
                const double aq0 = lut_aq[a0], aq1 = lut_aq[A + a1];
                const double a_eff = (NOISE && (rwv[seg] & 4u)) ? nav[seg] : a.env.a;
                double price = __dsub_rn(a_eff, __dmul_rn(a.env.b, __dadd_rn(aq0, aq1)));
                if (!(price > 0.0)) price = 0.0;
                const double r0d = __dmul_rn(price, aq0);
                const double r1d = __dmul_rn(price, aq1);
                if (seg == NSEG - 1) {
                    const int ll = T - 1 - seg * 64;       // lane of the episode's last step
                    last_price = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(price), ll),
                                                  __builtin_amdgcn_readlane(__double2loint(price), ll));
                }
                if (epk == 1) {
                    if (valid) {
                        lr0 += r0d; lr1 += r1d;          // divided by T once per episode below
                        la0 += lut_sct[a0]; la1 += lut_sct[A + a1];
                    }
                } else {
                    // several episodes per cycle: this segment's part of each episode's sums goes to that
                    // episode's accumulator slot (fixed point: exact whatever the split)
                    const int ep_l = min(tt, T - 1) / Tenv;
                    const int j0 = (seg * 64) / Tenv, j1 = (min(T, seg * 64 + 64) - 1) / Tenv;
                    const double s0 = lut_sct[a0], s1 = lut_sct[A + a1];
                    for (int j = j0; j <= j1; j++) {
                        const bool m = valid && ep_l == j;
                        log_into(e + j, m ? r0d : 0.0, m ? r1d : 0.0, m ? s0 : 0.0, m ? s1 : 0.0, j * Tenv >= seg * 64);
                    }
                }
                // visit counters (agents.py:76): the cell word goes to this wave's log (coalesced, L2-resident); the
                // counts are built per game below.  Only transitions still in the deque when it trains are counted.
                const bool trains = valid && tt >= replay_from;
                if (a.counter && !(kAblate & 32))
                    a.tlog[(((size_t)wave_gid * kWaveMaxEpisodes + e) * NSEG + seg) * 64 + lane] =
                        trains ? cwv[seg] : 0xFFFFFFFFu;

                // ---- replay schedule of this segment's 16 groups of four transitions, lane-parallel.
                //      Transition j may share a pass with an earlier transition i of its group unless it
                //      reads the row i writes (live next_max, agents.py:71) or rewrites i's cell (:75).
                //      A cut only counts between two transitions that both train (bit t of `pairs`: t - 1 and t do): the
                //      serial loop never looks at a cut at or in front of its first transition, or behind its last.
                //      cutq = the counted cut bits of the lane's group, in all four lanes of the quad.
                uint32_t P, cutq;
                bool any_fixed;
                //      (without CYCLE nothing is dropped in front, and step 0 is no cut position)
                const unsigned long long pairs = __ballot(CYCLE ? (valid && tt > replay_from) : valid);
                const uint32_t quad0 = (uint32_t)lane & 60u;
                if (kAblate & 128) { P = (act[seg] >> 24) * 0x204081u; any_fixed = false; cutq = 0u; }
                else if constexpr (kMaskSched) {
                    // x_i = my word ^ the word of position i of my quad (DPP folded into the xor): every test below is a
                    // byte-field zero test of x_i.  With d = my next row ^ my row, "my next row == its row" is
                    // byte 2 of x_i == d.  H_i = lanes with a hazard against position i (read by positions > i only).
                    const uint32_t w = act[seg];
                    const uint32_t d = (w >> 24) ^ ((w >> 16) & 0xFFu);
                    uint32_t x0 = w ^ dpp_src<0x00>(w), x1 = w ^ dpp_src<0x55>(w), x2 = w ^ dpp_src<0xAA>(w);
                    asm("" : "+v"(x0), "+v"(x1), "+v"(x2));       // (the fields are taken from x_i, not recomputed from the DPP value)
                    auto hz = [&](uint32_t x) -> unsigned long long {
                        const uint32_t xr = (x >> 16) & 0xFFu;
                        // same row, and a0 or a1 the same | next row == its row: one compare per ballot, ored as masks
                        return __ballot((((x & 0xFFu) * ((x >> 8) & 0xFFu)) | xr) == 0u) | __ballot(xr == d);
                    };
                    const unsigned long long H0 = hz(x0), H1 = hz(x1), H2 = hz(x2);
                    // cut bits of all 16 groups at once, as scalar arithmetic on the masks (bit 4g = group g)
                    const unsigned long long M = 0x1111111111111111ull;
                    const unsigned long long C1 = (H0 >> 1) & M;
                    const unsigned long long C2 = ((H1 >> 2) | ((H0 >> 2) & ~C1)) & M;
                    const unsigned long long C3 = ((H2 >> 3) | (((H1 >> 3) | ((H0 >> 3) & ~C1)) & ~C2)) & M;
                    // four identical transitions that stay in their row: position 3 equals positions 0-2, position 0 stays
                    const unsigned long long F = (__ballot((x0 | x1 | x2) == 0u) >> 3) & __ballot(d == 0u) & M;
                    const unsigned long long sched = (C1 & (pairs >> 1)) | ((C2 & (pairs >> 2)) << 1) | ((C3 & (pairs >> 3)) << 2) | (F << 3);
                    any_fixed = F != 0ull;
                    // the four next rows, 7 bits each: every lane shifts its own into place, two DPP ors collect the quad's
                    uint32_t rows = (w >> 24) << (7u * ((uint32_t)lane & 3u));
                    rows |= dpp_src<0xB1>(rows);                                   // quad_perm [1,0,3,2]
                    rows |= dpp_src<0x4E>(rows);                                   // quad_perm [2,3,0,1]
                    cutq = (uint32_t)(sched >> quad0);                             // bits 0-2 cuts, bit 3 fixed point, then the next group's
                    P = (cutq << 28) | rows;                                       // (read from lanes 4g only)
                } else {
                    const uint32_t w = act[seg];
                    const uint32_t b0 = dpp_mov32<0x00>(w), b1 = dpp_mov32<0x55>(w), b2 = dpp_mov32<0xAA>(w),
                                   b3 = dpp_mov32<0xFF>(w);                       // quad broadcasts of positions 0..3
                    const uint32_t qp = (uint32_t)lane & 3u;
                    auto hz = [&](uint32_t bi, uint32_t i) -> uint32_t {
                        const bool raw = (w >> 24) == ((bi >> 16) & 0xFFu);            // my next-state row == its written row
                        const bool waw = ((w >> 16) & 0xFFu) == ((bi >> 16) & 0xFFu) &&
                                         ((w & 0xFFu) == (bi & 0xFFu) || ((w >> 8) & 0xFFu) == ((bi >> 8) & 0xFFu));
                        return (qp > i && (raw || waw)) ? 1u : 0u;
                    };
                    const uint32_t hzw = hz(b0, 0u) | (hz(b1, 1u) << 1) | (hz(b2, 2u) << 2);
                    const uint32_t h1 = dpp_mov32<0x55>(hzw), h2 = dpp_mov32<0xAA>(hzw), h3 = dpp_mov32<0xFF>(hzw);
                    const uint32_t c1 = h1 & 1u;
                    const uint32_t c2 = ((h2 >> 1) & 1u) | ((c1 ^ 1u) & h2 & 1u);
                    const uint32_t c3 = ((h3 >> 2) & 1u) | ((c2 ^ 1u) & (((h3 >> 1) & 1u) | ((c1 ^ 1u) & h3 & 1u)));
                    // bit 31: the group runs in registers (replay_group): four identical transitions that stay in
                    // their row, or a period-2 cycle A, B, A, B between two different rows (told apart by rows 0 / 1)
                    // (the period-2 path only in the GREEDY variants: while the agents explore there are no such groups)
                    // NOISE: a noisy step that stays in its row has the SAME word as its neighbours but another reward
                    // (environments.py:29-33: the intercept is drawn), so its group must take the ordinary passes
                    bool quad_quiet = true;
                    if (NOISE) quad_quiet = ((__ballot((rwv[seg] & 4u) != 0u) >> (lane & 60)) & 0xFull) == 0ull;
                    const uint32_t same4 = ((quad_quiet && b0 == b1 && b1 == b2 && b2 == b3 && (b0 >> 24) == ((b0 >> 16) & 0xFFu)) ||
                                            (GREEDY && b0 == b2 && b1 == b3 && (b0 >> 24) == ((b1 >> 16) & 0xFFu) &&
                                             (b1 >> 24) == ((b0 >> 16) & 0xFFu) && (b0 >> 24) != (b1 >> 24))) ? 1u : 0u;
                    cutq = (c1 | (c2 << 1) | (c3 << 2)) & ((uint32_t)(pairs >> quad0) >> 1);
                    P = (b0 >> 24) | ((b1 >> 24) << 7) | ((b2 >> 24) << 14) | ((b3 >> 24) << 21) |
                        (cutq << 28) | (same4 << 31);
                    any_fixed = __ballot((P >> 31) != 0u) != 0ull;
                }

                // The replay key of this lane's transition: 4 * (its group's number in its 32-transition block) + the
                // number of its pass = the counted cuts in front of it in its group; kKeyNone if it does not train
                // (behind the cycle's end, or dropped from the deque).  It travels to the exec layout in the upper bits
                // of the store address (below 2^18), through the one ds_bpermute per block that the address takes anyway.
                const uint32_t pass_no = (uint32_t)__builtin_popcount(cutq & ((1u << ((uint32_t)lane & 3u)) - 1u));
                const uint32_t key_base = tab0_off + ((trains ? (quad0 & 28u) + pass_no : kKeyNone) << kKeyShift);
                const v2u woq = pack_halves(key_base + (cwv[seg] & 0xFFFFu) * kCellScale, key_base + (cwv[seg] >> 16) * kCellScale);

                // ---- (e) replay (agents.py:68-76): live next_max, writes in transition order
                // GREEDY variants: a converged game repeats ONE transition all segment long (a fixed point of the
                // greedy play) or cycles through TWO, THREE or FOUR.  Then train_net's loop is a recurrence on one cell
                // per cycle position and agent: the rows are read once, split into "the cell" and "the max of the rest",
                // and the segment's transitions run in registers -- two vector instructions each (cyclic_segment).
                bool seg_done = false;
                if (GREEDY && !(kAblate & 257) && !((explored_segs >> seg) & 1u)) {
                    const int nseg = min(64, T - seg * 64);
                    const uint32_t w = act[seg];
                    // smallest period p <= 4 of the segment's transition words (lane t against lane t - p)
                    const uint32_t w1 = dpp_mov32<0x138>(w), w2 = dpp_mov32<0x138>(w1);           // wave_shr:1, twice
                    const uint32_t w3 = dpp_mov32<0x138>(w2), w4 = dpp_mov32<0x138>(w3);
                    const bool in_seg = lane < nseg;
                    const int period = __ballot(in_seg && lane >= 1 && w != w1) == 0ull ? 1
                                     : __ballot(in_seg && lane >= 2 && w != w2) == 0ull ? 2
                                     : __ballot(in_seg && lane >= 3 && w != w3) == 0ull ? 3
                                     : __ballot(in_seg && lane >= 4 && w != w4) == 0ull ? 4 : 0;
                    if (period > 0 && nseg >= period) {
                        uint32_t W[4];
#pragma unroll
                        for (int j = 0; j < 4; j++) W[j] = readlane_u(w, j);
                        // the cycle must close (last -> first) and visit `period` DIFFERENT rows, so that every row
                        // holds exactly one of the rewritten cells
                        bool ok = true;
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (j < period) {
                                const uint32_t nxt_row = (W[(j + 1 < period) ? j + 1 : 0] >> 16) & 0xFFu;
                                ok = ok && (W[j] >> 24) == nxt_row;
#pragma unroll
                                for (int i = 0; i < j; i++) ok = ok && ((W[i] >> 16) & 0xFFu) != ((W[j] >> 16) & 0xFFu);
                            }
                        if (ok) {
                            seg_done = true;
                            const BlockOps<QT> ops0 = make_ops(snap[seg], 0, r0d, r1d, alpha_h);      // step layout: lane 32h + t
                            const unsigned tabh = half ? tab1_off : tab0_off;
                            const unsigned wo_step = woq.x & ((1u << kKeyShift) - 1u);            // (without the replay key)
                            if (period == 1) cyclic_segment<QT, 1>(ops0, wo_step, W, nseg, lane, tabh, A, row_bytes, ag_h, alpha_h, gamma_h);
                            else if (period == 2) cyclic_segment<QT, 2>(ops0, wo_step, W, nseg, lane, tabh, A, row_bytes, ag_h, alpha_h, gamma_h);
                            else if (period == 3) cyclic_segment<QT, 3>(ops0, wo_step, W, nseg, lane, tabh, A, row_bytes, ag_h, alpha_h, gamma_h);
                            else cyclic_segment<QT, 4>(ops0, wo_step, W, nseg, lane, tabh, A, row_bytes, ag_h, alpha_h, gamma_h);
                            __builtin_amdgcn_wave_barrier();
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (GREEDY && seg_done) break;
                    int nsub = __builtin_amdgcn_readfirstlane(min(32, T - seg * 64 - k * 32));
                    asm volatile("" : "+s"(nsub));          // (as for the play loop: keeps the per-group tests scalar compares)
                    if (nsub <= 0) break;
                    BlockOps<QT> ops = make_ops(snap[seg], k, r0d, r1d, alpha_h);
                    ops.permute(perm_sel);                                   // step layout -> exec layout
                    const unsigned wo = bperm(perm_sel, k ? woq.y : woq.x);
                    // 3 row reads per lane cover 24 columns (fewer columns: clamped duplicates), 4 cover 32.
                    // The fixed-point path is compiled into a second copy of the loop, entered only when the
                    // segment has such a group: the common exploring-regime loop stays as tight as without it.
#define THRL_REPLAY(RDN_, FP_) replay_block<QT, RDN_, FP_, kUnrollReplay && RDN_ == 3, GREEDY>(P, k * 32, nsub, ops, wo, rd_base, row_shift, my_step, row_bytes, \
                                                          ag_h, alpha_h, gamma_h, half != 0, seg * 64 + k * 32, replay_from)
                    if (A > 24)      { if (any_fixed) THRL_REPLAY(4, true); else THRL_REPLAY(4, false); }
                    else if (A >= 3) { if (any_fixed) THRL_REPLAY(3, true); else THRL_REPLAY(3, false); }
                    else             { if (any_fixed) THRL_REPLAY(2, true); else THRL_REPLAY(2, false); }
#undef THRL_REPLAY
                }
            }

            // ---- (f) per-episode log sums of this game into the wave accumulator:
            //      lane L gets the wave total of quantity L&3 = (reward0, reward1, action0, action1)
            //      kParkLogs: four lanes park the undivided totals for the game's epilogue instead.  wave_sum4's total is the
            //      same in all four rows but not in all lanes of a row (the rotate-adds associate differently by position), so
            //      the values parked are those of lanes 4 (e & 3) + k: bit for bit what lane 4 (e & 15) + k holds in log_into.
            if constexpr (kParkLogs) {
                const double v = (kAblate & 64) ? lr0 + lr1 + la0 + la1 : wave_sum4(lr0, lr1, la0, la1, lane);
                store_lanes(0xFull << (4 * (e & 3)), a.partial + ((size_t)wave_gid * kWaveMaxEpisodes + e) * 4, ((unsigned)lane & 3u) << 3, v);
            } else if (epk == 1) log_into(e, lr0, lr1, la0, la1, true);
            // epsilon decays after every train_net call (agents.py:78)
            if (SWEEP) {
                epsg0 = __dadd_rn(eend0, __dmul_rn(__dsub_rn(epsg0, eend0), estep0));
                epsg1 = __dadd_rn(eend1, __dmul_rn(__dsub_rn(epsg1, eend1), estep1));
            }
        }

        // ---- stream the windows back LDS -> HBM, store the env state
        {
            QT* d0 = q0 + lo * A;
            QT* d1 = q1 + lo * A;
            const int n = W * A;
            for (int k = lane; k < n; k += 64) { d0[k] = tab0[k]; d1[k] = tab1[k]; }
            if (spill0 >= 0 && lane < A) {
                q0[spill0 * A + lane] = tab0[W * A + lane];
                q1[spill0 * A + lane] = tab1[W * A + lane];
            }
            if (spill1 >= 0 && lane < A) {
                q0[spill1 * A + lane] = tab0[(W + 1) * A + lane];
                q1[spill1 * A + lane] = tab1[(W + 1) * A + lane];
            }
            if (lane == 0 && a.n_episodes > 0) a.state[g] = last_price;
            if (lane == 0 && sw_eps_on) { a.sw_eps[g] = epsg0; a.sw_eps[(size_t)a.G + g] = epsg1; }
        }
        __builtin_amdgcn_wave_barrier();

        // ---- visit counters of this game (agents.py:76).  The tables are back in HBM, so
        //      the wave's LDS region is free: build the launch's visit histogram there
        //      (one u32 per cell at the cell words' offsets, ds_add_u32 of 1) from the
        //      transition log, then add its non-zero cells to the counter window with no-return atomic adds
        //      (relaxed, agent scope): consecutive cells, so coalesced, and no load whose return the wave would
        //      have to wait for.  At most one add per cell, game and launch -- not one per transition
        //      (2e9 scattered atomics per launch were a 70 ms floor).
        const bool counting = a.counter && !(kAblate & 32);
        if constexpr (kParkLogs) {
            // ---- log sums of this game's episodes (no visit counters: a read-back of its own)
            if (!counting && a.n_episodes > 0) {
                const long long p0w = load_parked(0), p1w = load_parked(1);
                finish_parked(p0w, p1w);
            }
        }
        if (counting) {
            const int cells = (W + 2) * A;                       // per agent
            // may_alias: the histogram overlays the tables (no type-based reordering)
            typedef unsigned __attribute__((may_alias)) hist_u32;
            hist_u32* hist = reinterpret_cast<hist_u32*>(tab0);   // 2*cells dwords: agent 0's cells, then agent 1's
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            // (the region is 8-byte aligned: 2*cells dwords = cells 8-byte stores)
            for (int k = lane; k < cells; k += 64) lds_zero8(tab0_off + 8u * (unsigned)k);
            __builtin_amdgcn_wave_barrier();
            // log read-back: 4 episodes' loads in flight at a time (sc1 = L2-served: the wave
            // reads what it stored itself)
            const int n_cycles = a.n_episodes / epk;
            // kParkLogs: the game's parked log totals come back with the first batch (no round trip of their own)
            long long p0w = 0, p1w = 0;
            if constexpr (kParkLogs) { p0w = load_parked(0); p1w = load_parked(1); }
            for (int c0 = 0; c0 < n_cycles; c0 += 4) {
                unsigned w[4][NSEG];
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int seg = 0; seg < NSEG; seg++)
                        w[j][seg] = __hip_atomic_load(
                            &a.tlog[(((size_t)wave_gid * kWaveMaxEpisodes + min(c0 + j, n_cycles - 1) * epk) * NSEG + seg) * 64 + lane],
                            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int seg = 0; seg < NSEG; seg++) {
                        const unsigned ww = w[j][seg];
                        if (c0 + j < n_cycles && ww != 0xFFFFFFFFu) {
                            lds_inc(tab0_off + (ww & 0xFFFFu));
                            lds_inc(tab0_off + (ww >> 16));
                        }
                    }
            }
            if constexpr (kParkLogs) finish_parked(p0w, p1w);
            __builtin_amdgcn_wave_barrier();
            // apply: window rows are contiguous in HBM, so cell k of the window is element
            // lo*A + k of the agent's table (no row/column split); spill rows separately
            int32_t* cw0 = a.counter + (int64_t)g * a.stride + p0.table_off;
            int32_t* cw1 = a.counter + (int64_t)g * a.stride + p1.table_off;
            const int nwin = W * A;
            auto add = [](int32_t* p, unsigned n) {
                if (n) __hip_atomic_fetch_add(p, (int32_t)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            };
            for (int k = lane; k < nwin; k += 64) {
                add(cw0 + lo * A + k, hist[k]);
                add(cw1 + lo * A + k, hist[cells + k]);
            }
            if (lane < 2 * A) {
                const int which = lane >= A, col = lane - which * A;
                const int grow_ = which ? spill1 : spill0;
                if (grow_ >= 0) {
                    add(cw0 + grow_ * A + col, hist[nwin + lane]);
                    add(cw1 + grow_ * A + col, hist[cells + nwin + lane]);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    a.partial[(size_t)wave_gid * 128 + lane] = acc;
    a.partial[(size_t)wave_gid * 128 + 64 + lane] = acc_hi;
}

template <typename QT, int NSEG, int NRSEG, bool NOISE, bool SWEEP, bool CYCLE, bool GREEDY, bool LOG, bool AFFINE = false>
static int launch_wave_t(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    auto kern = k_wave_episodes<QT, NSEG, NRSEG, NOISE, SWEEP, CYCLE, GREEDY, LOG, AFFINE>;
    if (lds > 64 * 1024) {                       // beyond the default dynamic-LDS limit (float64 tables: one block per CU)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, a);
    return (int)hipGetLastError();
}

template <typename QT, bool NOISE, bool SWEEP, bool CYCLE, bool GREEDY, bool LOG>
static int launch_wave_nl(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    const int nseg = (a.T * a.epk + 63) / 64;
    const int nrseg = (a.win_rows + 2 + 63) / 64;
    if (nrseg == 1) {
        switch (nseg) {
            case 1: return launch_wave_t<QT, 1, 1, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 2: return launch_wave_t<QT, 2, 1, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 3: return launch_wave_t<QT, 3, 1, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 4: return launch_wave_t<QT, 4, 1, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
        }
    } else if (nrseg == 2) {
        switch (nseg) {
            case 1: return launch_wave_t<QT, 1, 2, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 2: return launch_wave_t<QT, 2, 2, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 3: return launch_wave_t<QT, 3, 2, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
            case 4: return launch_wave_t<QT, 4, 2, NOISE, SWEEP, CYCLE, GREEDY, LOG>(a, grid, block, lds, s);
        }
    }
    return -1;
}

template <typename QT, bool NOISE, bool SWEEP, bool CYCLE, bool GREEDY = false>
static int launch_wave_n(const WaveArgs& a, int grid, int block, size_t lds, hipStream_t s) {
    if (a.game_reward_log || a.game_action_log) return launch_wave_nl<QT, NOISE, SWEEP, CYCLE, GREEDY, true>(a, grid, block, lds, s);
    return launch_wave_nl<QT, NOISE, SWEEP, CYCLE, GREEDY, false>(a, grid, block, lds, s);
}

}  // namespace thrl
