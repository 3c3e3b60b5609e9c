// cfr.hip -- exact counterfactual regret minimisation on the enumerated tree: one iteration of up to 32 variants (plain CFR, CFR+, linear
// averaging, DCFR) in one top-down and one bottom-up sweep of the tree (gfx950).
//
// Sits next to: reg_evaluate.hip, whose two sweeps these are with the regret update in place of the logs.  Every state of these trees
// is its own information set for both players, so the tabular update is exact.  For member k with discounts (dp, dn, da) and side
// bits b, one call does, in this order of operations (-ffp-contract=off):
//   sigma[s,side,a] = R+(a) / sum R+  over the side's legal actions, a ascending, where the sum is > 0; else 1 / (number of legal actions);
//                     R+ = max(R, 0); 0 on illegal actions                                            (the regrets as they stand)
// top-down over level_order, reach[1] = (1, 1, 1), for every live link (s, r, c, t) -> u (chance > 0, next != 0):
//   reach_row[u] = reach_row[s] * sigma[s, r]     reach_col[u] = reach_col[s] * sigma[s, A + c]     reach_chance[u] = reach_chance[s] * chance
// bottom-up, V[0] = 0:
//   Q[s,r,c] = sum_t chance * (next == 0 ? value : values[next, k])                                   (chance <= 0 skipped)
//   q0[r] = sum_c Q[r,c] * sigma[A + c]      q1[c] = -(sum_r Q[r,c] * sigma[r])      v = sum_r sigma[r] * q0[r]      values[s,k] = v
//   for a side whose bit is set, on its legal actions, cf_row = reach_col * reach_chance, cf_col = reach_row * reach_chance:
//     R[a] <- (R[a] > 0 ? dp : dn) * R[a] + cf_side * (q_side[a] - v_side)       v_side = v (row), -v (column)
//     S[a] <- da * S[a] + own_reach_side * sigma_side[a]
// A side whose bit is clear, illegal actions, state 0 and states no live path reaches are never written in regret / strategy_sum.
// discount and sides are DEVICE arrays read by the kernels: a captured iteration follows them when the caller rewrites them.
//
// Work split, both sweeps, as k_reg_evaluate: one wave owns one state, lane = side * 32 + k owns one side of member k.  Top-down the
// lane forms its side's sigma from its A regrets, stores it, and hands its own-action reach on to every live child (the row lane the
// chance reach as well); the links are found 64 records at a time and walked off a ballot, as k_joint_reach does.  Bottom-up the state's
// records are staged once in the wave's LDS slice by a coalesced pass; the lane reads back the sigma the top-down sweep stored (the same
// bits on both sweeps), keeps its side's A regrets and sums in registers, and writes them back in place.  One cross-half shuffle: the
// row lane's v goes to the column lane.  The sides differ by selects only.  No atomics.
#include "tree_sweep.hpp"

using namespace rnad;
using namespace rnad::sweep;

namespace {

// Rows the sweeps never write -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in policy, values and reach
// (V[0] = 0 is in place when a record without a child selects row 0), and the root's three reach factors are 1.
__global__ __launch_bounds__(kThreads) void k_cfr_init(const int32_t *__restrict__ order_pos, int64_t S, int A2, int n,
                                                       float *__restrict__ policy, float *__restrict__ values, float *__restrict__ reach) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (s == 1) {
        for (int d = 0; d < 3 * n; ++d) reach[3 * n + d] = 1.0f;
        return;
    }
    if (order_pos[s] >= 0) return;
    for (int d = 0; d < n * A2; ++d) policy[s * n * A2 + d] = 0.0f;
    for (int k = 0; k < n; ++k) values[s * n + k] = 0.0f;
    for (int d = 0; d < 3 * n; ++d) reach[s * 3 * n + d] = 0.0f;
}

// One level, top-down: sigma of its states from the regrets as they stand, and the three reach factors of every live child.
// grid = ceil(n_states / kWaves).
template <int A>
__global__ __launch_bounds__(kThreads) void k_cfr_reach(const Trans *__restrict__ trans, const float *__restrict__ node, int C,
                                                        const int32_t *__restrict__ order, int64_t n_states, int n,
                                                        const float *__restrict__ regret, float *__restrict__ policy, float *reach) {
    constexpr int AA = A * A, NS = (AA + 2 + 3) & ~3;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t pos = (int64_t)blockIdx.x * kWaves + wave;
    if (pos >= n_states) return;
    const int s = order[pos];
    const int side = lane >> 5, k = lane & (kHalf - 1);
    const bool col_side = side != 0, on = k < n;
    const int kk = on ? k : 0;  // spare lanes shadow member 0 and store nothing
    const int64_t row_of = ((int64_t)s * n + kk) * (2 * A) + side * A;
    const float *nd = node + (int64_t)s * NS;
    const uint64_t bits = (uint64_t)__float_as_uint(nd[AA]) | ((uint64_t)__float_as_uint(nd[AA + 1]) << 32);
    float sig[A];
    float sum = 0.0f;
    int count = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const bool legal = ((bits >> (col_side ? a : a * A)) & 1) != 0;  // legal_tensor[s, 0, :, 0] and [s, 0, 0, :]
        const float r = regret[row_of + a];
        sig[a] = legal && r > 0.0f ? r : 0.0f;
        sum = legal ? sum + sig[a] : sum;
        count += legal ? 1 : 0;
    }
    const float uniform = 1.0f / (float)(count > 0 ? count : 1);
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const bool legal = ((bits >> (col_side ? a : a * A)) & 1) != 0;
        sig[a] = legal ? (sum > 0.0f ? sig[a] / sum : uniform) : 0.0f;
        if (on) policy[row_of + a] = sig[a];
    }
    const int64_t at = (int64_t)s * 3 * n;
    const float own = reach[at + side * n + kk], through_chance = reach[at + 2 * n + kk];
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
            const int mine = col_side ? rc % A : rc / A;
            float p = 0.0f;
#pragma unroll
            for (int a = 0; a < A; ++a) p = a == mine ? sig[a] : p;  // a select chain: no runtime-indexed array
            if (on) {
                reach[next * 3 * n + side * n + k] = own * p;
                if (!col_side) reach[next * 3 * n + 2 * n + k] = through_chance * chance;
            }
        }
    }
}

// One level, bottom-up: values of its states from the finished values below, then the regret and average-strategy update in place.
// grid = ceil(n_states / kWaves).
template <int A>
__global__ __launch_bounds__(kThreads) void k_cfr_update(const Trans *__restrict__ trans, const float *__restrict__ node, int C,
                                                         const int32_t *__restrict__ order, int64_t n_states, int n,
                                                         const float *__restrict__ discount, const int32_t *__restrict__ sides,
                                                         const float *__restrict__ policy, const float *__restrict__ reach,
                                                         float *__restrict__ regret, float *__restrict__ strategy_sum, float *values) {
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
    const int64_t row_of = ((int64_t)s * n + kk) * (2 * A);
    const float *ps = policy + row_of;
    float own[A], opp[A], R[A], T[A];  // the side's sigma, the sigma it answers, its regrets and its strategy sums
#pragma unroll
    for (int a = 0; a < A; ++a) {
        own[a] = ps[side * A + a];
        opp[a] = ps[(1 - side) * A + a];
        R[a] = regret[row_of + side * A + a];
        T[a] = strategy_sum[row_of + side * A + a];
    }
    const int64_t at = (int64_t)s * 3 * n;
    const float own_reach = reach[at + side * n + kk], opp_reach = reach[at + (1 - side) * n + kk], chance_reach = reach[at + 2 * n + kk];
    const float dp = discount[3 * kk], dn = discount[3 * kk + 1], da = discount[3 * kk + 2];
    const bool updates = ((sides[kk] >> side) & 1) != 0;
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
    float Q[AA];
    if (any_child)
        response_matrix<A, true>(rec, C, false, values + kk, n, Q);
    else
        response_matrix<A, false>(rec, C, false, values + kk, n, Q);

    // the lane's own action i against the other side's j, j ascending (k_reg_evaluate's order), then sum sigma q in action order
    float resp[A];
    float game = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        float r = 0.0f;
#pragma unroll
        for (int j = 0; j < A; ++j) r += (col_side ? Q[j * A + i] : Q[i * A + j]) * opp[j];
        resp[i] = col_side ? -r : r;
        game += own[i] * resp[i];
    }
    // the one exchange: the row lane's v goes to the column lane, which counts it as -v
    const float v_row = __shfl_xor(game, kHalf);
    const float v_side = col_side ? -v_row : game;
    if (!on) return;
    if (!col_side) values[(int64_t)s * n + k] = game;
    if (!updates) return;
    const float cf = opp_reach * chance_reach;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const bool legal = ((bits >> (col_side ? a : a * A)) & 1) != 0;
        const float kept = (R[a] > 0.0f ? dp : dn) * R[a];
        const float gain = cf * (resp[a] - v_side);
        const float played = own_reach * own[a];
        if (legal) {
            regret[row_of + side * A + a] = kept + gain;
            strategy_sum[row_of + side * A + a] = da * T[a] + played;
        }
    }
}

}  // namespace

extern "C" int64_t rnad_cfr_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return 3 * S * n;
}

extern "C" int rnad_cfr_iterate(const rnad_tree_t *tree, int n, const float *discount, const int32_t *sides, float *regret,
                                float *strategy_sum, float *policy, float *values, float *reach, void *stream_) {
    RNAD_REQUIRE(tree && discount && sides && regret && strategy_sum && policy && values && reach, "rnad_cfr_iterate: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_cfr_iterate: %d members outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->node && tree->NS == node_stride_floats(tree->A) && tree->level_order && tree->order_pos &&
                     tree->n_levels >= 1 && tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_cfr_iterate: bad tree");
    {  // no in/out or output buffer may overlap another buffer anywhere, not only at its first byte
        const size_t column = (size_t)tree->S * (size_t)n * sizeof(float), table = column * 2 * (size_t)tree->A;
        const struct { const char *p; size_t n; } buf[7] = {{(const char *)discount, (size_t)n * 3 * sizeof(float)}, {(const char *)sides, (size_t)n * sizeof(int32_t)},
                                                             {(const char *)regret, table}, {(const char *)strategy_sum, table},
                                                             {(const char *)policy, table}, {(const char *)values, column}, {(const char *)reach, 3 * column}};
        for (int i = 0; i < 7; ++i)
            for (int j = (i < 2 ? 2 : i + 1); j < 7; ++j)
                RNAD_REQUIRE(buf[i].p + buf[i].n <= buf[j].p || buf[j].p + buf[j].n <= buf[i].p,
                             i < 2 ? "rnad_cfr_iterate: a table or an output overlaps discount or sides" : "rnad_cfr_iterate: two tables or outputs overlap");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_cfr_iterate: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_cfr_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tree->order_pos, tree->S,
                       2 * tree->A, n, policy, values, reach);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = 0; l < tree->n_levels; ++l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_cfr_reach<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                                   tree->node, tree->C, tree->level_order + off, cnt, n, regret, policy, reach);
        }
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_cfr_update<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                                   tree->node, tree->C, tree->level_order + off, cnt, n, discount, sides, policy, reach, regret, strategy_sum,
                                   values);
        }
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
