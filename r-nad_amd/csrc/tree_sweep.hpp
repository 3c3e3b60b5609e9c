// tree_sweep.hpp -- what the wave-per-state sweeps over [S][n][2A] policy tables share: best_response.hip and reg_evaluate.hip.
//
//   response_matrix   the state's A x A matrix of one member from records staged in LDS and the finished rows below (bottom-up);
//   k_joint_reach     one level of table k's joint reach, chance included, handed on to every live child (top-down).
// Both files launch these very functions, so the reach of rnad_best_response and of rnad_reg_evaluate carries the same bits.
#pragma once
#include "common.hpp"

namespace rnad {
namespace sweep {
namespace {  // a copy per translation unit: each file's code object holds the kernels it launches

constexpr int kWaves = 4, kThreads = 64 * kWaves, kHalf = 32;
static_assert(RNAD_CROSS_PLAY_MAX == kHalf, "a half-wave holds one side's members");

// Per joint action the chance outcomes in order, as k_best_response sums them: m += (payoff or the child's value) * chance.  No branch: a
// record without chance adds nothing through a select, and with CHILD a record that leaves the tree (or has no chance) reads row 0 of
// the table below -- zeros, written by the caller's init kernel earlier on the stream -- and discards it (k_cross_play's scheme).
// negate: the lane counts a terminal payoff as -value (the column side of a best response).
template <int A, bool CHILD>
__device__ __forceinline__ void response_matrix(const uint32_t *rec, int C, bool negate, const float *below, int stride,
                                                float (&m)[A * A]) {
    constexpr int AA = A * A;
#pragma unroll
    for (int rc = 0; rc < AA; ++rc) m[rc] = 0.0f;
    for (int t = 0; t < C; ++t) {
#pragma unroll
        for (int rc = 0; rc < AA; ++rc) {
            const uint32_t *x = rec + (rc * C + t) * 3;  // {next, chance, value}: the same address in every lane
            const float chance = __uint_as_float(x[1]), value = __uint_as_float(x[2]);
            const bool live = chance > 0.0f;
            float v = negate ? -value : value;  // terminal: row_b, col_b = v, -v (metric.py:141-144)
            if (CHILD) {
                const int next = live ? (int)x[0] : 0;
                const float child = below[(int64_t)next * stride];
                v = next == 0 ? v : child;
            }
            m[rc] = live ? m[rc] + v * chance : m[rc];
        }
    }
}

// One level, top-down: a wave per state hands the reach of its n tables on to every live child, n consecutive floats per child.  A tree
// has one live link per state on average among its A * A * C records: the lanes look at 64 records at a time, read straight from the
// table (coalesced; nothing is read twice, so nothing is staged), and the wave walks the set bits of the ballot, as k_mixture does.  Lane
// k < n carries table k.  A thread per (state, table) that walks all records itself was measured at 5.50 ms against 3.00 ms on the
// configs[3]-shaped tree at n = 32 (profiles/best_response_variants.md).
template <int A>
__global__ __launch_bounds__(kThreads) void k_joint_reach(const Trans *__restrict__ trans, int C, const int32_t *__restrict__ order,
                                                          int64_t n_states, int n, const float *__restrict__ policies, float *reach) {
    constexpr int AA = A * A;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t pos = (int64_t)blockIdx.x * kWaves + wave;
    if (pos >= n_states) return;
    const int s = order[pos];
    const bool on = lane < n;
    const int k = on ? lane : 0;
    const float rs = reach[(int64_t)s * n + k];
    const float *ps = policies + ((int64_t)s * n + k) * (2 * A);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(trans + (int64_t)s * AA * C);
    for (int base = 0; base < AA * C; base += 64) {
        const int d = base + lane;
        const bool in = d < AA * C;
        const int next_l = in ? (int)src[3 * d] : 0;
        const float chance_l = in ? __uint_as_float(src[3 * d + 1]) : 0.0f;
        const bool live = next_l != 0 && chance_l > 0.0f;
        for (uint64_t todo = __ballot(live); todo != 0; todo &= todo - 1) {
            const int bit = __ffsll((unsigned long long)todo) - 1, rc = (base + bit) / C;
            const int64_t next = __shfl(next_l, bit);
            const float chance = __shfl(chance_l, bit);
            const float through = rs * (ps[rc / A] * ps[A + rc % A]);
            if (on) reach[next * n + k] = through * chance;
        }
    }
}

// The top-down half of a call: one k_joint_reach launch per level; reach[1] = 1 and the zero rows are the caller's init kernel's.
template <int A>
inline void launch_joint_reach(const rnad_tree_t *tree, int n, const float *policies, float *reach, hipStream_t stream) {
    for (int l = 0; l < tree->n_levels; ++l) {
        const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
        if (cnt > 0)
            hipLaunchKernelGGL((k_joint_reach<A>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                               tree->C, tree->level_order + off, cnt, n, policies, reach);
    }
}

}  // namespace
}  // namespace sweep
}  // namespace rnad
