// best_response.hip -- the best response to each of n policy tables, as a policy, with where on the tree it gains (gfx950).
//
// Sits next to: the bottom-up half of nashconv.hip (k_best_response, util/metric.py:134-175), which gives the best-response VALUES of
// one table, and cross_play.hip / mixture.hip, whose [S][n][2A] tables, level launches and LDS staging this file shares.  For member k,
// side 0 is the row player responding to k's column side, side 1 the column player responding to k's row side:
//   m[s, r, c]        = sum_t chance[s,t,r,c] * (next == 0 ? +-value[s,t,r,c] : values[next, side, k])     (chance <= 0 skipped;
//                                                                                                          side 1's terminal payoff is -value)
//   q[s, 0, k, r]     = sum_c m[s, r, c] * J_k[s, A + c]            q[s, 1, k, c] = sum_r J_k[s, r] * m[s, r, c]
//   values[s, side, k] = max over the side's legal a of q          (strict > in ascending order: ties go to the lowest legal index)
//   best[s, k, side*A + a] = 1 at that a, 0 elsewhere
//   gain[s, side, k]  = values[s, side, k] - sum over legal a of J_k[s, side*A + a] * q[s, side, k, a]
//   reach[1, k] = 1,  reach[u, k] = reach[s, k] * (J_k[s, r] * J_k[s, A + c]) * chance       for every live link (s, r, c, t) -> u
// `reach` is table k's JOINT reach, chance included, in the orientation of cross_play.hip (the row action weighted with the row player's
// policy); it is NOT the pi[A + r] * pi[c] product that k_reach (nashconv.hip) keeps from the reference.  With it the
// performance-difference identity holds per side: exploitability_side(k) = sum_s reach[s, k] * gain[s, side, k].
// The sums keep the order of k_best_response operation by operation (the build has -ffp-contract=off), so values[:, 0, k] and
// values[:, 1, k] carry the bits of rnad_nashconv's row_best and col_best for table k.
//
// Work split, bottom-up: one wave owns one state, lane = side * 32 + k owns one side of member k (the half-wave split of k_mixture).
// The state's Trans records are staged in the wave's LDS slice with one pass of coalesced loads and read back at lane-uniform addresses,
// as in k_cross_play: the transition table is read once per 32 opponents, not once per opponent.  A child's values are two runs of n
// consecutive floats.  The two sides differ only in which policy half they read, in the sign of a terminal payoff and in whether the
// lane's own action is the row or the column of m: selects, no divergent branch.  Top-down: a wave per state, a lane per member.
// response_matrix and the top-down kernel (k_joint_reach) live in tree_sweep.hpp, which reg_evaluate.hip shares.
#include "tree_sweep.hpp"

using namespace rnad;
using namespace rnad::sweep;

namespace {

// Rows the sweeps never write -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in all four outputs, and the
// root's reach is 1.  A kernel, not a memset node: see zero_async in common.hpp.
__global__ __launch_bounds__(kThreads) void k_best_response_init(const int32_t *__restrict__ order_pos, int64_t S, int A2, int n,
                                                                 float *__restrict__ best, float *__restrict__ values,
                                                                 float *__restrict__ gain, float *__restrict__ reach) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (s == 1) {
        for (int k = 0; k < n; ++k) reach[n + k] = 1.0f;
        return;
    }
    if (order_pos[s] >= 0) return;
    for (int d = 0; d < n * A2; ++d) best[s * n * A2 + d] = 0.0f;
    for (int d = 0; d < 2 * n; ++d) values[s * 2 * n + d] = gain[s * 2 * n + d] = 0.0f;
    for (int k = 0; k < n; ++k) reach[s * n + k] = 0.0f;
}

// One level, bottom-up: the four outputs' rows of its states from the finished levels below.  grid = ceil(n_states / kWaves).
template <int A>
__global__ __launch_bounds__(kThreads) void k_best_response_sweep(const Trans *__restrict__ trans, const float *__restrict__ node, int C,
                                                                  const int32_t *__restrict__ order, int64_t n_states, int n,
                                                                  const float *__restrict__ policies, float *__restrict__ best,
                                                                  float *values, float *__restrict__ gain) {
    constexpr int AA = A * A, NS = (AA + 2 + 3) & ~3;
    static_assert(sizeof(Trans) == 12, "records are staged as three words");
    __shared__ uint32_t staged[kWaves][AA * RNAD_MAX_TRANSITIONS * 3];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t pos = (int64_t)blockIdx.x * kWaves + wave;
    const bool active = pos < n_states;
    const int s = active ? order[pos] : 0;  // a spare wave of the last block stages state 0 and stores nothing
    const int side = lane >> 5, k = lane & (kHalf - 1);
    const bool col_side = side != 0, on = k < n;
    const int kk = on ? k : 0;  // spare lanes shadow member 0 and store nothing
    // the lane's own loads are issued before the records': they depend on nothing but s
    const float *ps = policies + ((int64_t)s * n + kk) * (2 * A);
    float own[A], opp[A];  // the responding side's entries of table k (for the gain), and the side it responds to
#pragma unroll
    for (int a = 0; a < A; ++a) {
        own[a] = ps[side * A + a];
        opp[a] = ps[(1 - side) * A + a];
    }
    const float *nd = node + (int64_t)s * NS;
    const uint64_t bits = (uint64_t)__float_as_uint(nd[AA]) | ((uint64_t)__float_as_uint(nd[AA + 1]) << 32);
    uint32_t *rec = staged[wave];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(trans + (int64_t)s * AA * C);
        for (int d = lane; d < AA * C * 3; d += 64) rec[d] = src[d];
    }
    __syncthreads();
    if (!active) return;
    bool child = false;
    for (int d = lane; d < AA * C; d += 64) child |= rec[3 * d] != 0 && __uint_as_float(rec[3 * d + 1]) > 0.0f;
    const bool any_child = __ballot(child) != 0;  // the same in every lane
    const int slot = side * n + kk;
    float m[AA];
    if (any_child)
        response_matrix<A, true>(rec, C, col_side, values + slot, 2 * n, m);
    else
        response_matrix<A, false>(rec, C, col_side, values + slot, 2 * n, m);
    // the lane's own action i against the other side's j: rowr[r] += mr * pi[A + c] over c, colr[c] += pi[r] * mc over r (nashconv.hip)
    float top = -INFINITY, played = 0.0f;
    int arg = -1;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        float resp = 0.0f;
#pragma unroll
        for (int j = 0; j < A; ++j) resp += (col_side ? m[j * A + i] : m[i * A + j]) * opp[j];
        const bool legal = ((bits >> (col_side ? i : i * A)) & 1) != 0;  // legal_tensor[s, 0, :, 0] and [s, 0, 0, :] (metric.py:167-168)
        const bool better = legal && resp > top;
        top = better ? resp : top;
        arg = better ? i : arg;
        played = legal ? played + own[i] * resp : played;
    }
    if (!on) return;
    values[(int64_t)s * (2 * n) + slot] = top;
    gain[(int64_t)s * (2 * n) + slot] = top - played;
    float *row = best + ((int64_t)s * n + k) * (2 * A) + side * A;
#pragma unroll
    for (int a = 0; a < A; ++a) row[a] = a == arg ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int64_t rnad_best_response_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return 2 * S * n;
}

extern "C" int rnad_best_response(const rnad_tree_t *tree, int n, const float *policies, float *best, float *values, float *gain,
                                  float *reach, void *stream_) {
    RNAD_REQUIRE(tree && policies && best && values && gain && reach, "rnad_best_response: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_best_response: %d policies outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->node && tree->NS == node_stride_floats(tree->A) && tree->level_order && tree->order_pos &&
                     tree->n_levels >= 1 && tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_best_response: bad tree");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_best_response: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_best_response_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       tree->order_pos, tree->S, 2 * tree->A, n, best, values, gain, reach);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_best_response_sweep<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream,
                                   tree->trans, tree->node, tree->C, tree->level_order + off, cnt, n, policies, best, values, gain);
        }
        launch_joint_reach<kA>(tree, n, policies, reach, stream);
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
