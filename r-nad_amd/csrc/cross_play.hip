// cross_play.hip -- exact payoff of every pair of n policies on the whole tree, one bottom-up sweep (gfx950).
//
// Sits next to: util/metric.py:134-175 (the bottom-up half of NashConvData.get_nashconv), which evaluates ONE joint policy
// against its best responses.  Here policy i plays the rows and policy j the columns, for all n * n pairs at once:
//   V[s, i, j] = sum_{r,c} J_i[s, r] * J_j[s, A + c] * sum_t chance[s,t,r,c] * (next == 0 ? value[s,t,r,c] : V[next, i, j])
// The orientation -- the row action weighted with the row player's policy -- is that of metric.py:169-170 (matmul(M_row, pi_col),
// matmul(pi_row, M_col)).  It is NOT the pi_col[r] * pi_row[c] product of the reference's reach sweep (metric.py:130-132), which
// k_reach (nashconv.hip) reproduces on purpose.  V is the row player's payoff, the column player's is -V.  Citations are
// baskuit/R-NaD file:line.
//
// Work split: one wave owns one state and one tile of 64 pairs p = i * n + j, one pair per lane.  The state's Trans records are
// the same for every lane: the wave loads them once, coalesced, into its slice of LDS and reads them back at lane-uniform addresses.
// A child's values are 64 consecutive floats of its row: one coalesced 256-byte read per tile.  The transition table is read once
// per tile of 64 pairs instead of once per pair.  With fewer than 64 pairs (n < 8) the spare lanes stay idle: packing
// several states into a wave would make the record addresses differ across lanes and turn every record fetch into a gather, and the
// records, not the lanes, are what the sweep pays for.
#include "common.hpp"

using namespace rnad;

namespace {

constexpr int kWaves = 4, kThreads = 64 * kWaves;

// Rows the sweep never writes -- the absorbing state 0 and states no chance > 0 path reaches -- are zero.  A kernel, not a memset
// node: see zero_async in common.hpp.
__global__ __launch_bounds__(kThreads) void k_cross_play_zero(const int32_t *__restrict__ order_pos, int64_t S, int P,
                                                              float *__restrict__ values) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S || order_pos[s] >= 0) return;
    float *row = values + s * P;
    for (int p = 0; p < P; ++p) row[p] = 0.0f;
}

// The sums of one state for one lane's pair from the state's staged records: per joint action the chance outcomes in order, then the
// joint actions c inside r, one accumulator -- a fixed order, no atomics: the same inputs give the same bits.
// There is no branch: a record without chance adds nothing through a select, and with CHILD a record that leaves the tree (or has no
// chance) reads row 0 of `values` -- zeros, written by k_cross_play_zero earlier on the stream -- and discards it.  So the A * A record
// reads and the A * A child reads of one chance outcome are in flight together instead of one behind the other's branch.
template <int A, bool CHILD>
__device__ __forceinline__ float cross_play_state(const uint32_t *rec, int C, const float (&pr)[A], const float (&pc)[A],
                                                  const float *below, int P) {
    constexpr int AA = A * A;
    float m[AA];  // per joint action: sum_t chance * (payoff or child value)
#pragma unroll
    for (int rc = 0; rc < AA; ++rc) m[rc] = 0.0f;
    for (int t = 0; t < C; ++t) {
#pragma unroll
        for (int rc = 0; rc < AA; ++rc) {
            const uint32_t *x = rec + (rc * C + t) * 3;  // {next, chance, value}: the same address in every lane
            const float chance = __uint_as_float(x[1]), value = __uint_as_float(x[2]);
            const bool live = chance > 0.0f;  // as k_best_response: entries without chance are skipped
            float v = value;
            if (CHILD) {
                const int next = live ? (int)x[0] : 0;
                const float child = below[(int64_t)next * P];
                v = next == 0 ? value : child;
            }
            m[rc] = live ? m[rc] + chance * v : m[rc];
        }
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < A; ++r) {
#pragma unroll
        for (int c = 0; c < A; ++c) acc += (pr[r] * pc[c]) * m[r * A + c];
    }
    return acc;
}

// One level: values of its states from the finished levels below.  grid = (ceil(n_states / kWaves), tiles of 64 pairs).
// A wave copies the 12 * A * A * C bytes of its state's records into its own LDS slice with one pass of coalesced loads -- the only
// time the wave touches the table -- and every lane then reads each record from the same LDS address.  A state none of whose
// records leads to a child (the deepest level, and every pruned branch above it) reads nothing from `values`.
template <int A>
__global__ __launch_bounds__(kThreads) void k_cross_play(const Trans *__restrict__ trans, int C, const int32_t *__restrict__ order,
                                                         int64_t n_states, int n, const float *__restrict__ policies, float *values) {
    constexpr int AA = A * A;
    static_assert(sizeof(Trans) == 12, "records are staged as three words");
    __shared__ uint32_t staged[kWaves][AA * RNAD_MAX_TRANSITIONS * 3];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int P = n * n;
    const int64_t k = (int64_t)blockIdx.x * kWaves + wave;
    const bool active = k < n_states;
    const int s = active ? order[k] : 0;  // a spare wave of the last block stages state 0 and stores nothing
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
    const int p = (int)blockIdx.y * 64 + lane;
    const bool on = p < P;
    const int q = on ? p : P - 1;  // spare lanes of the last tile shadow the last pair and store nothing
    const int i = q / n, j = q - i * n;
    // the state's n * 2A policy floats are contiguous; a lane keeps the 2A it needs in registers
    const float *ps = policies + (int64_t)s * n * (2 * A);
    float pr[A], pc[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        pr[a] = ps[i * (2 * A) + a];
        pc[a] = ps[j * (2 * A) + A + a];
    }
    const float *below = values + q;
    const float acc = any_child ? cross_play_state<A, true>(rec, C, pr, pc, below, P) : cross_play_state<A, false>(rec, C, pr, pc, below, P);
    if (on) values[(int64_t)s * P + p] = acc;
}

}  // namespace

extern "C" int64_t rnad_cross_play_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return S * n * n;
}

extern "C" int rnad_cross_play(const rnad_tree_t *tree, int n, const float *policies, float *values, void *stream_) {
    RNAD_REQUIRE(tree && policies && values, "rnad_cross_play: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_cross_play: %d policies outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->level_order && tree->order_pos && tree->n_levels >= 1 &&
                     tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_cross_play: bad tree");
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_cross_play: cannot select device %d", tree->device);
    const int P = n * n, tiles = (P + 63) / 64;
    hipLaunchKernelGGL(k_cross_play_zero, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tree->order_pos,
                       tree->S, P, values);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_cross_play<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves), (unsigned)tiles), dim3(kThreads), 0,
                                   stream, tree->trans, tree->C, tree->level_order + off, cnt, n, policies, values);
        }
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
