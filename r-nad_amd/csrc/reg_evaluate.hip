// reg_evaluate.hip -- exact policy evaluation in the regularised game: values, action values, fixed-point residual and reach of up to 32
// (policy, magnet, eta) triples in one bottom-up and one top-down sweep of the tree (gfx950).
//
// Sits next to: reg_solve.hip, which finds the fixed point of a magnet; this file says how far an ARBITRARY policy is from it, and what it
// is worth on the way.  It is what the learner estimates by sampling (V-trace on transformed rewards, learn/vtrace.py:234-239) with the
// samples taken out.  For member k (policy pi_k, log magnet lm_k, eta_k > 0), bottom-up over level_order, V[0] = 0:
//   Q[s,r,c]       = sum_t chance[s,t,r,c] * (next == 0 ? value[s,t,r,c] : values[next, k])            (chance <= 0 skipped)
//   q[s,k,r]       = sum_c Q[s,r,c] * pi_k[s, A + c]            q[s,k,A + c] = - sum_r pi_k[s, r] * Q[s,r,c]
//   KL_side        = sum over a with pi > 0 of pi[a] * (log pi[a] - lm[a])                               (a select, never 0 * inf)
//   values[s,k]    = sum_r pi_k[s,r] * q[s,k,r] - eta_k * KL_row + eta_k * KL_col
//   residual[s,k]  = max over both sides and the side's support (legal, lm > -inf) of |pi(a) - softmax(lm + q / eta_k)(a)|
// q is the unregularised response, the column player's in its OWN payoff (the sign of reg_solve.hip's `responses`); the logs enter only
// values and residual.  The residual is reg_solve.hip's stopping quantity, operation by operation (residual_of there).  Top-down:
//   reach[1,k] = 1,   reach[u,k] = reach[s,k] * (pi_k[s,r] * pi_k[s,A+c]) * chance        for every live link
// by the kernel rnad_best_response launches (tree_sweep.hpp): the same bits.  Nothing checks that pi is absolutely continuous with respect
// to the magnet: pi > 0 where lm = -inf gives KL = +inf by plain arithmetic (learn.tabular.evaluate_regularized refuses such input).
//
// Work split, bottom-up, as k_best_response_sweep: one wave owns one state, lane = side * 32 + k owns one side of member k.  The state's
// records are staged once in the wave's LDS slice by a coalesced pass and read back at lane-uniform addresses; a child's values are one
// run of n consecutive floats.  The lane keeps its side's A policy and A log-magnet entries and the other side's A policy entries in
// registers.  One cross-half shuffle: the column lane sends its KL, the row lane its residual; the row lane then stores values, the
// column lane the residual, each lane its side's half of q.  The sides differ by selects only.  eta: n kernel arguments.
#include "tree_sweep.hpp"

#include <cmath>

using namespace rnad;
using namespace rnad::sweep;

namespace {

struct Etas {
    float v[RNAD_CROSS_PLAY_MAX];
};

// Rows the sweeps never write -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in all four outputs (V[0] = 0 is
// in place when a record without a child selects row 0), and the root's reach is 1.  A kernel, not a memset node (zero_async, common.hpp).
__global__ __launch_bounds__(kThreads) void k_reg_evaluate_init(const int32_t *__restrict__ order_pos, int64_t S, int A2, int n,
                                                                float *__restrict__ values, float *__restrict__ q,
                                                                float *__restrict__ residual, float *__restrict__ reach) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (s == 1) {
        for (int k = 0; k < n; ++k) reach[n + k] = 1.0f;
        return;
    }
    if (order_pos[s] >= 0) return;
    for (int d = 0; d < n * A2; ++d) q[s * n * A2 + d] = 0.0f;
    for (int k = 0; k < n; ++k) values[s * n + k] = residual[s * n + k] = reach[s * n + k] = 0.0f;
}

// One level, bottom-up: values, q and residual of its states from the finished values below.  grid = ceil(n_states / kWaves).
template <int A>
__global__ __launch_bounds__(kThreads) void k_reg_evaluate(const Trans *__restrict__ trans, const float *__restrict__ node, int C,
                                                           const int32_t *__restrict__ order, int64_t n_states, int n, const Etas etas,
                                                           const float *__restrict__ policies, const float *__restrict__ log_reg,
                                                           float *values, float *__restrict__ q, float *__restrict__ residual) {
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
    const float *ps = policies + row_of, *ls = log_reg + row_of + side * A;
    float own[A], opp[A], lm[A];  // the side's own policy and log magnet, and the policy of the side it answers
#pragma unroll
    for (int a = 0; a < A; ++a) {
        own[a] = ps[side * A + a];
        opp[a] = ps[(1 - side) * A + a];
        lm[a] = ls[a];
    }
    const float eta = etas.v[kk];
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

    // the lane's own action i against the other side's j, j ascending: Q[r][c] * pi[A + c] over c, pi[r] * Q[r][c] over r (reg_solve.hip's
    // `responses`; its qc -= p * Q and the negated sum carry the same bits).  Then the side's support, its KL and sum pi q in action order.
    const float inv_eta = 1.0f / eta;
    float resp[A], t[A];
    float game = 0.0f, kl = 0.0f, top = -INFINITY;
    unsigned sup = 0;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        float r = 0.0f;
#pragma unroll
        for (int j = 0; j < A; ++j) r += (col_side ? Q[j * A + i] : Q[i * A + j]) * opp[j];
        resp[i] = col_side ? -r : r;
        const bool legal = ((bits >> (col_side ? i : i * A)) & 1) != 0;  // legal_tensor[s, 0, :, 0] and [s, 0, 0, :]
        const bool in = legal && lm[i] > -INFINITY;
        sup |= (unsigned)in << i;
        game += own[i] * resp[i];
        const bool played = own[i] > 0.0f;
        const float term = own[i] * (logf(played ? own[i] : 1.0f) - lm[i]);
        kl = played ? kl + term : kl;
        t[i] = (in ? lm[i] : 0.0f) + resp[i] * inv_eta;
        top = in && t[i] > top ? t[i] : top;
    }
    // max_a |pi(a) - softmax(lm + q / eta)(a)| over the support: residual_of of reg_solve.hip
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        t[i] = ((sup >> i) & 1) ? expf(t[i] - top) : 0.0f;
        sum += t[i];
    }
    float res = 0.0f;
#pragma unroll
    for (int i = 0; i < A; ++i) {
        const float d = fabsf(own[i] - t[i] / sum);
        res = ((sup >> i) & 1) && d > res ? d : res;
    }
    // the one exchange: the column lane's KL goes to the row lane, the row lane's residual to the column lane
    const float other = __shfl_xor(col_side ? kl : res, kHalf);
    if (!on) return;
    const int64_t slot = (int64_t)s * n + k;
    float *row = q + slot * (2 * A) + side * A;
#pragma unroll
    for (int a = 0; a < A; ++a) row[a] = resp[a];
    if (col_side)
        residual[slot] = fmaxf(other, res);
    else
        values[slot] = game - eta * kl + eta * other;
}

}  // namespace

extern "C" int64_t rnad_reg_evaluate_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return S * n;
}

extern "C" int rnad_reg_evaluate(const rnad_tree_t *tree, int n, const float *eta, const float *policies, const float *log_reg, float *values,
                                 float *q, float *residual, float *reach, void *stream_) {
    RNAD_REQUIRE(tree && eta && policies && log_reg && values && q && residual && reach, "rnad_reg_evaluate: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_reg_evaluate: %d policies outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    Etas etas = {};
    for (int k = 0; k < RNAD_CROSS_PLAY_MAX; ++k) {
        etas.v[k] = k < n ? eta[k] : 1.0f;
        RNAD_REQUIRE(etas.v[k] > 0.0f && std::isfinite(etas.v[k]),
                     "rnad_reg_evaluate: eta[%d] = %g is not a positive number (the unregularised game has no fixed point to measure against)", k,
                     (double)etas.v[k]);
    }
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->node && tree->NS == node_stride_floats(tree->A) && tree->level_order && tree->order_pos &&
                     tree->n_levels >= 1 && tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_reg_evaluate: bad tree");
    {  // no output may overlap an input or another output anywhere, not only at its first byte
        const size_t column = (size_t)tree->S * (size_t)n * sizeof(float), table = column * 2 * (size_t)tree->A;
        const struct { const char *p; size_t n; } buf[6] = {{(const char *)policies, table}, {(const char *)log_reg, table}, {(const char *)values, column},
                                                             {(const char *)q, table},        {(const char *)residual, column}, {(const char *)reach, column}};
        for (int i = 0; i < 6; ++i)
            for (int j = (i < 2 ? 2 : i + 1); j < 6; ++j)
                RNAD_REQUIRE(buf[i].p + buf[i].n <= buf[j].p || buf[j].p + buf[j].n <= buf[i].p,
                             i < 2 ? "rnad_reg_evaluate: an output overlaps an input" : "rnad_reg_evaluate: two outputs overlap");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_reg_evaluate: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_reg_evaluate_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tree->order_pos,
                       tree->S, 2 * tree->A, n, values, q, residual, reach);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_reg_evaluate<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                                   tree->node, tree->C, tree->level_order + off, cnt, n, etas, policies, log_reg, values, q, residual);
        }
        launch_joint_reach<kA>(tree, n, policies, reach, stream);
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
