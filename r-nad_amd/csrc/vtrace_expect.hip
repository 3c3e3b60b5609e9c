// vtrace_expect.hip -- the exact EXPECTED learner update: what the two-player V-trace targets and action values of learn/vtrace.py are in
// expectation over complete episodes played by a behaviour table mu, for up to 32 members at once, in one bottom-up and one top-down sweep
// of the tree (gfx950).
//
// Sits next to: reg_evaluate.hip, which evaluates a policy; this file evaluates the ESTIMATOR -- clips rho and c, lambda, gamma, the
// bootstrap from the target net's value vv and the evaluated policy pip = pi_processed differing from the behaviour mu.  Member k has its
// own tables (mu, pip, lpol [S][n][2A], vv [S][n][2]) and its own (eta, gamma, lambda, rho, c), which travel as kernel arguments.  With
// cs = pip / mu (mu = 0: never drawn, skipped), e[P] = sum_a pip lpol of side P, g = gamma, lgg = (lambda g) g, r the payoff of a record
// that leaves the tree, n its child otherwise, p its chance (p <= 0 skipped), bottom-up over level_order:
//   row side (0, s), w = cs0[a] cs1[b]:
//     W0      = vv0 + sum_{a,b} (mu0[a] mu1[b]) (min(w, rho) (((g eta) e1 - eta e0 - vv0) + g T[a,b]) + lgg min(w, c) U[a,b])
//               T = sum_t p (leaves ? r : g vv0[n])          U = sum_t p (leaves ? 0 : W0[n] - vv0[n])
//     q[0][a] = ((g eta) e1 - eta lpol0[a]) + g sum_b pip1[b] sum_t p (leaves ? r : g W0[n])
//   column side (1, s), given the row action a:
//     W1[a]   = vv1 + sum_b mu1[b] sum_t p (leaves ? min(cs1[b], rho) ((-r - eta e1) - vv1)
//                                                  : sum_a' mu0[n][a'] (min(w', rho) X + lgg min(w', c) (W1[n][a'] - vv1[n])))
//               w' = cs1[b] cs0[n][a']                      X = (((g eta) e0[n] - eta e1) + (g g) vv1[n]) - vv1
//     q[1][b] = - eta lpol1[b] + sum_a mu0[a] sum_t p (leaves ? -r : (g eta) e0[n] + (g g) sum_a' pip0[n][a'] W1[n][a'])
//   target[0] = W0, target[1] = sum_a mu0[a] W1[a], target_given_row = W1.  An action the behaviour never draws (mu = 0) keeps what the
//   sampled program leaves there: q = vv - eta lpol.
// Top-down: reach under mu by k_joint_reach (tree_sweep.hpp), the kernel rnad_best_response launches: the same bits.
//
// Work split, as k_reg_evaluate: one wave owns one state, lane = side * 32 + k one side of member k; the records are staged once in the
// wave's LDS slice and read back at lane-uniform addresses; the sides differ by selects, but for the column side's A-fold sum over the
// child's row actions, which only the column half-wave walks.  What a parent reads of a child is ONE export record that the child wrote:
// workspace [S][3A + 5][n], field-major so that the 32 members of a field are one run of n floats:
//   0 vv0   1 W0   2 e0   3 vv1   4 sum_a' pip0 W1   5 .. mu0[A]   5 + A .. cs0[A]   5 + 2A .. (W1 - vv1)[A]
// The row lane writes fields 0 - 2 and mu0, cs0; the column lane the rest.  One cross-half shuffle (each side's e).
#include "tree_sweep.hpp"

#include <cmath>

using namespace rnad;
using namespace rnad::sweep;

namespace {

struct Hyper {  // per member, by value: a captured call keeps them
    float eta[RNAD_CROSS_PLAY_MAX], gamma[RNAD_CROSS_PLAY_MAX], lambda[RNAD_CROSS_PLAY_MAX], rho[RNAD_CROSS_PLAY_MAX], c[RNAD_CROSS_PLAY_MAX];
};

constexpr int export_fields(int A) { return 3 * A + 5; }

// Rows the sweeps never write -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in the outputs and in the export
// workspace (a record without a child selects row 0 and discards it), and the root's reach is 1.
__global__ __launch_bounds__(kThreads) void k_vtrace_expect_init(const int32_t *__restrict__ order_pos, int64_t S, int A, int n,
                                                                 float *__restrict__ target, float *__restrict__ given_row,
                                                                 float *__restrict__ q, float *__restrict__ reach,
                                                                 float *__restrict__ ws) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (s == 1) {
        for (int k = 0; k < n; ++k) reach[n + k] = 1.0f;
        return;
    }
    if (order_pos[s] >= 0) return;
    const int F = export_fields(A);
    for (int d = 0; d < n * 2 * A; ++d) q[s * n * 2 * A + d] = 0.0f;
    for (int d = 0; d < n * A; ++d) given_row[s * n * A + d] = 0.0f;
    for (int d = 0; d < n * 2; ++d) target[s * n * 2 + d] = 0.0f;
    for (int k = 0; k < n; ++k) reach[s * n + k] = 0.0f;
    for (int d = 0; d < n * F; ++d) ws[s * n * F + d] = 0.0f;
}

// One level, bottom-up.  grid = ceil(n_states / kWaves).  CHILD = false: no record of the state leads to a child, nothing below is read.
template <int A, bool CHILD>
__device__ __forceinline__ void vtrace_expect_state(const uint32_t *rec, int C, int n, int k, bool on, bool col_side, int64_t s, float eta,
                                                    float g, float lam, float rho, float cbar, const float (&mu_own)[A],
                                                    const float (&pip_own)[A], const float (&lpol_own)[A], const float (&mu_opp)[A],
                                                    const float (&pip_opp)[A], float vv, float *__restrict__ target,
                                                    float *__restrict__ given_row, float *__restrict__ q, float *ws) {
    constexpr int F = export_fields(A);
    // the side's entropy term and ratios; e crosses the half-waves once
    float e_own = 0.0f, cs_own[A], cs_opp[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        e_own = pip_own[a] > 0.0f ? e_own + pip_own[a] * lpol_own[a] : e_own;
        cs_own[a] = mu_own[a] > 0.0f ? pip_own[a] / mu_own[a] : 0.0f;
        cs_opp[a] = mu_opp[a] > 0.0f ? pip_opp[a] / mu_opp[a] : 0.0f;
    }
    const float e_opp = __shfl_xor(e_own, kHalf);
    const float e0 = col_side ? e_opp : e_own, e1 = col_side ? e_own : e_opp;
    const float ge = g * eta, gg = g * g, lgg = (lam * g) * g;
    const float base0 = (ge * e1 - eta * e0) - vv;  // the row side's clipped term without the transition
    float acc = 0.0f, qa[A], wa[A];                 // row: W0 - vv0;  q by own action;  column: W1[a] - vv1 by row action
#pragma unroll
    for (int a = 0; a < A; ++a) qa[a] = wa[a] = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int b = 0; b < A; ++b) {
            // row lane: own action a, the other side's b; column lane: own b, the other side's a
            const float mu0a = col_side ? mu_opp[a] : mu_own[a], mu1b = col_side ? mu_own[b] : mu_opp[b];
            const float cs1b = col_side ? cs_own[b] : cs_opp[b], cs0a = col_side ? 0.0f : cs_own[a];
            const float pip1b = col_side ? pip_own[b] : pip_opp[b];
            const float leave_clip = fminf(cs1b, rho);
            float x = 0.0f, y = 0.0f, z = 0.0f;  // row: T, U and q's tail;  column: W1's and q's sums over the chance outcomes
            for (int t = 0; t < C; ++t) {
                const uint32_t *r3 = rec + ((a * A + b) * C + t) * 3;  // {next, chance, value}: the same address in every lane
                const float chance = __uint_as_float(r3[1]), value = __uint_as_float(r3[2]);
                const bool live = chance > 0.0f;
                float tx = 0.0f, ux = 0.0f, zx = 0.0f;
                bool leaves = true;
                if (CHILD) {
                    const int next = live ? (int)r3[0] : 0;
                    leaves = next == 0;
                    const float *below = ws + (int64_t)next * F * n + k;
                    const float f_a = below[(col_side ? 3 : 0) * n], f_b = below[(col_side ? 4 : 1) * n], e0n = below[2 * n];
                    // row: f_a = vv0[n], f_b = W0[n];  column: f_a = vv1[n], f_b = sum_a' pip0 W1
                    float inner = 0.0f;
                    if (col_side && !leaves) {
                        const float X = (((ge * e0n - eta * e1) + gg * f_a) - vv);
#pragma nounroll
                        for (int i = 0; i < A; ++i) {
                            const float m = below[(5 + i) * n], c0 = below[(5 + A + i) * n], d = below[(5 + 2 * A + i) * n];
                            const float w = cs1b * c0;
                            const float term = fminf(w, rho) * X + lgg * fminf(w, cbar) * d;
                            inner = m > 0.0f ? inner + m * term : inner;
                        }
                    }
                    tx = col_side ? inner : g * f_a;
                    ux = col_side ? 0.0f : f_b - f_a;
                    zx = col_side ? ge * e0n + gg * f_b : g * f_b;
                }
                const float tl = col_side ? leave_clip * ((-value - eta * e1) - vv) : value;
                const float zl = col_side ? -value : value;
                tx = leaves ? tl : tx;
                ux = leaves ? 0.0f : ux;
                zx = leaves ? zl : zx;
                x = live ? x + chance * tx : x;
                y = live ? y + chance * ux : y;
                z = live ? z + chance * zx : z;
            }
            const float w = cs0a * cs1b;
            const float term = fminf(w, rho) * (base0 + g * x) + lgg * fminf(w, cbar) * y;
            const bool both = mu0a > 0.0f && mu1b > 0.0f;
            acc = both ? acc + (mu0a * mu1b) * term : acc;
            const float zr = mu1b > 0.0f ? qa[a] + pip1b * z : qa[a];  // the row side's tail: cs1[b] mu1[b] = pip1[b]
            const float zc = mu0a > 0.0f ? qa[b] + mu0a * z : qa[b];
            const float wc = mu1b > 0.0f ? wa[a] + mu1b * x : wa[a];
            if (col_side) {
                qa[b] = zc;
                wa[a] = wc;
            } else {
                qa[a] = zr;
            }
        }
    }
    // results and the export record for the parent
    float w1[A], tgt = 0.0f, p1 = 0.0f, qout[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        w1[a] = vv + wa[a];
        tgt = mu_opp[a] > 0.0f ? tgt + mu_opp[a] * w1[a] : tgt;
        p1 = mu_opp[a] > 0.0f ? p1 + pip_opp[a] * w1[a] : p1;
        const float lead = col_side ? -(eta * lpol_own[a]) : ge * e1 - eta * lpol_own[a];
        const float drawn = lead + (col_side ? qa[a] : g * qa[a]);
        qout[a] = mu_own[a] > 0.0f ? drawn : vv - eta * lpol_own[a];
    }
    if (!on) return;
    const float w0 = vv + acc;
    const int64_t slot = s * n + k;
    target[slot * 2 + (col_side ? 1 : 0)] = col_side ? tgt : w0;
    float *qrow = q + slot * (2 * A) + (col_side ? A : 0);
#pragma unroll
    for (int a = 0; a < A; ++a) qrow[a] = qout[a];
    float *mine = ws + s * F * n + k;
    if (col_side) {
        mine[3 * n] = vv;
        mine[4 * n] = p1;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            given_row[slot * A + a] = w1[a];
            mine[(5 + 2 * A + a) * n] = wa[a];  // W1 - vv1 without the round trip through W1
        }
    } else {
        mine[0] = vv;
        mine[n] = w0;
        mine[2 * n] = e0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            mine[(5 + a) * n] = mu_own[a];
            mine[(5 + A + a) * n] = cs_own[a];
        }
    }
}

template <int A>
__global__ __launch_bounds__(kThreads) void k_vtrace_expect(const Trans *__restrict__ trans, int C, const int32_t *__restrict__ order,
                                                            int64_t n_states, int n, const Hyper hyper, const float *__restrict__ mu,
                                                            const float *__restrict__ pip, const float *__restrict__ lpol,
                                                            const float *__restrict__ vvs, float *__restrict__ target,
                                                            float *__restrict__ given_row, float *__restrict__ q, float *ws) {
    constexpr int AA = A * A;
    static_assert(sizeof(Trans) == 12, "records are staged as three words");
    __shared__ uint32_t staged[kWaves][AA * RNAD_MAX_TRANSITIONS * 3];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int64_t pos = (int64_t)blockIdx.x * kWaves + wave;
    const bool active = pos < n_states;
    const int s = active ? order[pos] : 0;  // a spare wave of the last block stages state 0 and stores nothing
    const int side = lane >> 5, k = lane & (kHalf - 1);
    const bool col_side = side != 0, on = k < n;
    const int kk = on ? k : 0;  // spare lanes shadow member 0 and store nothing
    const int64_t row_of = ((int64_t)s * n + kk) * (2 * A);
    float mu_own[A], pip_own[A], lpol_own[A], mu_opp[A], pip_opp[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        mu_own[a] = mu[row_of + side * A + a];
        pip_own[a] = pip[row_of + side * A + a];
        lpol_own[a] = lpol[row_of + side * A + a];
        mu_opp[a] = mu[row_of + (1 - side) * A + a];
        pip_opp[a] = pip[row_of + (1 - side) * A + a];
    }
    const float vv = vvs[((int64_t)s * n + kk) * 2 + side];
    const float eta = hyper.eta[kk], g = hyper.gamma[kk], lam = hyper.lambda[kk], rho = hyper.rho[kk], cbar = hyper.c[kk];
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
    if (any_child)
        vtrace_expect_state<A, true>(rec, C, n, kk, on, col_side, s, eta, g, lam, rho, cbar, mu_own, pip_own, lpol_own, mu_opp, pip_opp, vv,
                                     target, given_row, q, ws);
    else
        vtrace_expect_state<A, false>(rec, C, n, kk, on, col_side, s, eta, g, lam, rho, cbar, mu_own, pip_own, lpol_own, mu_opp, pip_opp, vv,
                                      target, given_row, q, ws);
}

}  // namespace

extern "C" int64_t rnad_vtrace_expect_size(int64_t S, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX) return -1;
    return S * n;
}

extern "C" int64_t rnad_vtrace_expect_workspace(int64_t S, int A, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX || A < 1 || A > RNAD_MAX_ACTIONS) return -1;
    return S * n * export_fields(A);
}

extern "C" int rnad_vtrace_expect(const rnad_tree_t *tree, int n, const float *hyper, const float *mu, const float *pip, const float *lpol,
                                  const float *vv, float *target, float *target_given_row, float *q, float *reach, float *workspace,
                                  void *stream_) {
    RNAD_REQUIRE(tree && hyper && mu && pip && lpol && vv && target && target_given_row && q && reach && workspace,
                 "rnad_vtrace_expect: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_vtrace_expect: %d members outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2, "rnad_vtrace_expect: a tree of %lld states has no root", (long long)tree->S);
    Hyper h = {};
    for (int k = 0; k < RNAD_CROSS_PLAY_MAX; ++k) {
        const float *x = hyper + 5 * (k < n ? k : 0);
        h.eta[k] = x[0], h.gamma[k] = x[1], h.lambda[k] = x[2], h.rho[k] = x[3], h.c[k] = x[4];
        RNAD_REQUIRE(std::isfinite(x[0]) && std::isfinite(x[2]), "rnad_vtrace_expect: eta[%d] = %g or lambda[%d] = %g is not finite", k,
                     (double)x[0], k, (double)x[2]);
        RNAD_REQUIRE(x[1] > 0.0f && std::isfinite(x[1]), "rnad_vtrace_expect: gamma[%d] = %g is not a positive number", k, (double)x[1]);
        RNAD_REQUIRE(x[3] >= 0.0f && x[4] >= 0.0f, "rnad_vtrace_expect: the clips rho[%d] = %g, c[%d] = %g must not be negative", k,
                     (double)x[3], k, (double)x[4]);
    }
    RNAD_REQUIRE(tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS && tree->trans &&
                     tree->level_order && tree->order_pos && tree->n_levels >= 1 &&
                     tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_vtrace_expect: bad tree");
    {  // no output may overlap an input or another output anywhere, not only at its first byte
        const size_t column = (size_t)tree->S * (size_t)n * sizeof(float), A = (size_t)tree->A, table = column * 2 * A;
        const struct { const char *p; size_t n; } buf[9] = {
            {(const char *)mu, table},          {(const char *)pip, table},     {(const char *)lpol, table},
            {(const char *)vv, column * 2},     {(const char *)target, column * 2}, {(const char *)target_given_row, column * A},
            {(const char *)q, table},           {(const char *)reach, column},  {(const char *)workspace, column * (size_t)export_fields(tree->A)}};
        for (int i = 0; i < 9; ++i)
            for (int j = (i < 4 ? 4 : i + 1); j < 9; ++j)
                RNAD_REQUIRE(buf[i].p + buf[i].n <= buf[j].p || buf[j].p + buf[j].n <= buf[i].p,
                             i < 4 ? "rnad_vtrace_expect: an output overlaps an input" : "rnad_vtrace_expect: two outputs overlap");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_vtrace_expect: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_vtrace_expect_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, tree->order_pos,
                       tree->S, tree->A, n, target, target_given_row, q, reach, workspace);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_vtrace_expect<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, tree->trans,
                                   tree->C, tree->level_order + off, cnt, n, h, mu, pip, lpol, vv, target, target_given_row, q, workspace);
        }
        launch_joint_reach<kA>(tree, n, mu, reach, stream);
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
