// mixture.hip -- the behaviour policy that plays like a mixture of n whole policies, one top-down sweep of the tree (gfx950).
//
// Sits next to: cross_play.hip, and walks the same tables in the same orientation (the row action weighted with the row player's
// policy, util/metric.py:169-170).  A mixture "draw member k with probability w[k], then play J_k to the end" is not the state-wise
// average of the tables: by Kuhn's theorem the equivalent behaviour policy weights member k at state s with the probability that
// k's OWN actions lead to s,
//   reach[1, side, k] = 1
//   reach[u, 0, k]    = reach[s, 0, k] * J_k[s, r]          for every live link (s, r, c, t) -> u  (chance > 0, next != 0)
//   reach[u, 1, k]    = reach[s, 1, k] * J_k[s, A + c]
//   D[s, side]        = sum_k w[side, k] * reach[s, side, k]
//   mix[s, side*A+a]  = sum_k w[side, k] * reach[s, side, k] * J_k[s, side*A + a] / D[s, side]        where D > 0
//                     = sum_k w[side, k] * J_k[s, side*A + a]                                          where D == 0
// (D == 0: the mixture's own player never comes to s, nothing at the root depends on the row; it is kept a distribution.)
// This is NOT k_reach (nashconv.hip): that sweep carries one table's JOINT reach, chance included, in the reference's
// pi[A + r] * pi[c] orientation.  Here neither the opponent's action nor chance enters, and the tree must be a tree: a state with two
// parents has no own-action reach (util.metric.mixture checks that; this file cannot look at device data).
//
// Work split: one wave owns one state, lane = side * 32 + k owns member k of one side and keeps its reach and its A policy entries in
// registers.  The state's Trans records are staged in the wave's LDS slice with one pass of coalesced loads, as in k_cross_play.  Each
// side sums inside its half-wave with xor-shuffles of 16, 8, 4, 2, 1 (spare lanes add 0): a fixed butterfly, no atomics, no branch on D
// -- the same inputs give the same bits.  For every live link the wave stores the 2n consecutive floats of the child's reach row; a
// tree has one live link per state on average, so the lanes test 64 records at a time and the wave walks the ballot's set bits
// instead of all A * A * C records.
#include "common.hpp"

using namespace rnad;

namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves, kHalf = 32;
static_assert(RNAD_CROSS_PLAY_MAX == kHalf, "a half-wave holds one side's members");

// Rows the sweep never writes -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in both outputs, and the
// root's reach is 1.  A kernel, not a memset node: see zero_async in common.hpp.
__global__ __launch_bounds__(kThreads) void k_mixture_init(const int32_t *__restrict__ order_pos, int64_t S, int A2, int n2,
                                                           float *__restrict__ mix, float *__restrict__ reach) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (s == 1) {
        for (int d = 0; d < n2; ++d) reach[n2 + d] = 1.0f;
        return;
    }
    if (order_pos[s] >= 0) return;
    for (int d = 0; d < A2; ++d) mix[s * A2 + d] = 0.0f;
    for (int d = 0; d < n2; ++d) reach[s * n2 + d] = 0.0f;
}

// the sum over the lanes of one half-wave, in every lane of it
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int m = kHalf / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One level: the mixture at its states from the reach rows the level above stored, and the reach rows of its children.
// grid = ceil(n_states / kWaves).  The stream orders this level's stores before the next level's loads.
template <int A>
__global__ __launch_bounds__(kThreads) void k_mixture(const Trans *__restrict__ trans, int C, const int32_t *__restrict__ order,
                                                      int64_t n_states, int n, const float *__restrict__ policies,
                                                      const float *__restrict__ weights, float *__restrict__ mix, float *reach) {
    constexpr int AA = A * A;
    static_assert(sizeof(Trans) == 12, "records are staged as three words");
    __shared__ uint32_t staged[kWaves][AA * RNAD_MAX_TRANSITIONS * 3];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t pos = (int64_t)blockIdx.x * kWaves + wave;
    const bool active = pos < n_states;
    const int s = active ? order[pos] : 0;  // a spare wave of the last block stages state 0 and stores nothing
    const int side = lane >> 5, k = lane & (kHalf - 1);
    const bool on = k < n;
    const int slot = side * n + (on ? k : 0);  // spare lanes shadow member 0, contribute 0 and store nothing
    float *own = reach + (int64_t)s * (2 * n);
    const float rk = on ? own[slot] : 0.0f;
    const float w = on ? weights[slot] : 0.0f;
    const float *ps = policies + ((int64_t)s * n + (on ? k : 0)) * (2 * A) + side * A;
    float p[A];
#pragma unroll
    for (int a = 0; a < A; ++a) p[a] = on ? ps[a] : 0.0f;
    // (the lane's own loads are issued before the records': they depend on nothing but s, and behind the barrier they would wait for it)
    uint32_t *rec = staged[wave];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(trans + (int64_t)s * AA * C);
        for (int d = lane; d < AA * C * 3; d += 64) rec[d] = src[d];
    }
    __syncthreads();
    if (!active) return;
    // the A + 1 sums of the lane's side, and the A sums of the D == 0 row
    const float wr = w * rk;
    const float D = half_sum(wr);
    float out = 0.0f;  // lane k < A of a side ends up with mix[s, side * A + k]
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float num = half_sum(wr * p[a]), flat = half_sum(w * p[a]);
        const float m = D > 0.0f ? num / D : flat;
        out = k == a ? m : out;
    }
    if (k < A) mix[(int64_t)s * (2 * A) + side * A + k] = out;
    // reach of the children: the lane's own action of the link, nothing of the opponent's and nothing of chance.  A tree has one live
    // link per state on average among its A * A * C records: the lanes look at 64 records at a time, and the wave walks the live ones
    for (int base = 0; base < AA * C; base += 64) {
        const int d = base + lane;
        const bool live = d < AA * C && rec[3 * d] != 0 && __uint_as_float(rec[3 * d + 1]) > 0.0f;
        for (uint64_t todo = __ballot(live); todo != 0; todo &= todo - 1) {  // the same in every lane
            const int link = base + __ffsll((unsigned long long)todo) - 1, rc = link / C;
            const int64_t next = (int)rec[3 * link];
            const float v = rk * ps[side ? rc % A : rc / A];  // (a second read of an entry of p: the index is not known at compile time)
            if (on) reach[next * (2 * n) + slot] = v;
        }
    }
}

}  // namespace

extern "C" int64_t rnad_mixture_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return 2 * S * n;
}

extern "C" int rnad_mixture(const rnad_tree_t *tree, int n, const float *policies, const float *weights, float *mix, float *reach,
                            void *stream_) {
    RNAD_REQUIRE(tree && policies && weights && mix && reach, "rnad_mixture: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_mixture: %d policies outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->level_order && tree->order_pos && tree->n_levels >= 1 &&
                     tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_mixture: bad tree");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_mixture: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_mixture_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tree->order_pos,
                       tree->S, 2 * tree->A, 2 * n, mix, reach);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = 0; l < tree->n_levels; ++l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_mixture<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                                   tree->C, tree->level_order + off, cnt, n, policies, weights, mix, reach);
        }
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
