// vtrace_moments.hip -- the exact VARIANCE of the learner's estimates: the second central moments of the two-player V-trace targets and of
// the action values q over complete episodes played by a behaviour table mu, for up to 32 members at once, in one bottom-up sweep of the
// tree (gfx950).
//
// Sits next to: vtrace_expect.hip, which gives the first moments.  This file runs AFTER a completed rnad_vtrace_expect on the same inputs
// and takes every first moment from it -- its outputs target, target_given_row, q and its export record [S][3A + 5][n] (fields 0 vv0,
// 1 W0, 2 e0, 3 vv1, 5 .. mu0[A], 5 + A .. cs0[A], 5 + 2A .. (W1 - vv1)[A]) -- and recomputes none of them.  Given the joint action and the
// chance outcome everything random in a sampled target is the child's sampled target, so with d0 = W0 - vv0, dW1[a] = W1[a] - vv1,
// lgg = (lambda g) g, u the child of a record, r its payoff otherwise, p its chance (p <= 0 skipped, as every term with mu = 0):
//   row side, w = cs0[a] cs1[b], delta0 = (g eta e1 - eta e0 - vv0) + g (u ? g vv0[u] : r):
//     dev      = (min(w, rho) delta0 + (u ? lgg min(w, c) d0[u] : 0)) - d0[s]
//     V0[s]    = sum_{a,b} (mu0[a] mu1[b]) sum_t p (dev^2 + (u ? (lgg min(w, c))^2 V0[u] : 0))
//     tm       = (g eta e1 + g cs1[b] (u ? g W0[u] : r)) - vv0,        tbar[a] = q[0][a] - (vv0 - eta lpol0[a])
//     q_var[0][a] = (sum_b mu1[b] sum_t p ((tm - tbar[a])^2 + (u ? (g g cs1[b])^2 V0[u] : 0)) + (1 - mu0[a]) tbar[a]^2) / mu0[a]
//   column side given the row action a, w' = cs1[b] cs0[u][a'], X = ((g eta e0[u] - eta e1) + g g vv1[u]) - vv1:
//     dev'     = (min(w', rho) X + lgg min(w', c) dW1[u][a']) - dW1[s][a]
//     V1[s][a] = sum_b mu1[b] sum_t p (u ? sum_a' mu0[u][a'] (dev'^2 + (lgg min(w', c))^2 V1[u][a'])
//                                        : (min(cs1[b], rho) ((-r - eta e1) - vv1) - dW1[s][a])^2),     0 where mu0[a] = 0
//     tm'      = u ? (g eta e0[u] + g g cs0[u][a'] (vv1[u] + dW1[u][a'])) - vv1 : -r - vv1,     tbar'[b] = q[1][b] - (vv1 - eta lpol1[b])
//     q_var[1][b] = (sum_a mu0[a] sum_t p (u ? sum_a' mu0[u][a'] ((tm' - tbar'[b])^2 + (g g cs0[u][a'])^2 V1[u][a']) : (tm' - tbar'[b])^2)
//                    + (1 - mu1[b]) tbar'[b]^2) / mu1[b]
//   target_var[0] = V0, target_given_row_var = V1, target_var[1] = sum_a mu0[a] (V1[a] + (W1[a] - target[1])^2); q_var = 0 where mu = 0.
// Every summand is a square or a product of squares: nothing is formed as E[x^2] - E[x]^2.
//
// Work split, as k_vtrace_expect: one wave owns one state, lane = side * 32 + k one side of member k; the records are staged once in the
// wave's LDS slice and read back at lane-uniform addresses; the column half-wave alone walks the child's A entries.  What a parent reads
// of a child's second moments is ONE export record the child wrote: workspace [S][A + 1][n], field-major (0 V0, 1 .. V1[A]).
#include "tree_sweep.hpp"

#include <cmath>

using namespace rnad;
using namespace rnad::sweep;

namespace {

struct Hyper {  // per member, by value: a captured call keeps them
    float eta[RNAD_CROSS_PLAY_MAX], gamma[RNAD_CROSS_PLAY_MAX], lambda[RNAD_CROSS_PLAY_MAX], rho[RNAD_CROSS_PLAY_MAX], c[RNAD_CROSS_PLAY_MAX];
};

constexpr int first_fields(int A) { return 3 * A + 5; }
constexpr int moment_fields(int A) { return A + 1; }

// Rows the sweep never writes -- the absorbing state 0 and states no chance > 0 path reaches -- are zero in the outputs and in the export
// workspace (a record without a child selects row 0 and discards it).
__global__ __launch_bounds__(kThreads) void k_vtrace_moments_init(const int32_t *__restrict__ order_pos, int64_t S, int A, int n,
                                                                  float *__restrict__ target_var, float *__restrict__ given_row_var,
                                                                  float *__restrict__ q_var, float *__restrict__ ws) {
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= S) return;
    if (order_pos[s] >= 0) return;
    const int F = moment_fields(A);
    for (int d = 0; d < n * 2 * A; ++d) q_var[s * n * 2 * A + d] = 0.0f;
    for (int d = 0; d < n * A; ++d) given_row_var[s * n * A + d] = 0.0f;
    for (int d = 0; d < n * 2; ++d) target_var[s * n * 2 + d] = 0.0f;
    for (int d = 0; d < n * F; ++d) ws[s * n * F + d] = 0.0f;
}

// One state.  CHILD = false: no record of the state leads to a child, nothing below is read.
template <int A, bool CHILD>
__device__ __forceinline__ void vtrace_moments_state(const uint32_t *rec, int C, int n, int k, bool on, bool col_side, int64_t s, float eta,
                                                     float g, float lam, float rho, float cbar, const float (&mu_own)[A],
                                                     const float (&mu_opp)[A], const float (&cs_own)[A], const float (&cs_opp)[A],
                                                     const float (&tbar)[A], float e0, float e1, float vv, float tgt,
                                                     const float *__restrict__ first, const float *__restrict__ given_row,
                                                     float *__restrict__ target_var, float *__restrict__ given_row_var,
                                                     float *__restrict__ q_var, float *ws) {
    constexpr int F1 = first_fields(A), F2 = moment_fields(A);
    const float ge = g * eta, gg = g * g, lgg = (lam * g) * g;
    const float base0 = (ge * e1 - eta * e0) - vv;  // the row side's clipped term without the transition
    const float lead0 = ge * e1;
    const float d0s = tgt - vv;  // row lane: W0 - vv0
    float dw1s[A];               // column lane: (W1 - vv1)[a] of the own record
#pragma unroll
    for (int a = 0; a < A; ++a) dw1s[a] = first[(s * F1 + 5 + 2 * A + a) * n + k];
    float acc = 0.0f, qv[A], va[A];  // row: V0;  the q sums by own action;  column: V1[a] by row action
#pragma unroll
    for (int a = 0; a < A; ++a) qv[a] = va[a] = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
        for (int b = 0; b < A; ++b) {
            // row lane: own action a, the other side's b; column lane: own b, the other side's a
            const float mu0a = col_side ? mu_opp[a] : mu_own[a], mu1b = col_side ? mu_own[b] : mu_opp[b];
            const float cs1b = col_side ? cs_own[b] : cs_opp[b], cs0a = col_side ? 0.0f : cs_own[a];
            const float w = cs0a * cs1b;
            const float cr = col_side ? fminf(cs1b, rho) : fminf(w, rho);  // column: the clip of a record that leaves
            const float cc = lgg * fminf(w, cbar), cc2 = cc * cc;
            const float gc = g * cs1b, ggc = gg * cs1b, ggc2 = ggc * ggc;
            const float tb = col_side ? tbar[b] : tbar[a];
            const float dws = dw1s[a];
            float x = 0.0f, z = 0.0f;  // the target's and q's sums over the chance outcomes
            for (int t = 0; t < C; ++t) {
                const uint32_t *r3 = rec + ((a * A + b) * C + t) * 3;  // {next, chance, value}: the same address in every lane
                const float chance = __uint_as_float(r3[1]), value = __uint_as_float(r3[2]);
                const bool live = chance > 0.0f;
                int next = 0;
                if (CHILD) next = live ? (int)r3[0] : 0;
                const bool leaves = next == 0;
                float tx, zx;
                if (col_side) {
                    const float devl = cr * ((-value - eta * e1) - vv) - dws;
                    const float dql = (-value - vv) - tb;
                    tx = devl * devl;
                    zx = dql * dql;
                    if (CHILD && !leaves) {
                        const float *below = first + (int64_t)next * F1 * n + k;
                        const float *mom = ws + (int64_t)next * F2 * n + k;
                        const float e0n = below[2 * n], vv1n = below[3 * n];
                        const float lead = ge * e0n;
                        const float X = ((lead - eta * e1) + gg * vv1n) - vv;
                        float inner = 0.0f, innerq = 0.0f;
#pragma nounroll
                        for (int i = 0; i < A; ++i) {
                            const float m = below[(5 + i) * n], c0 = below[(5 + A + i) * n], d = below[(5 + 2 * A + i) * n];
                            const float vc = mom[(1 + i) * n];
                            const float wp = cs1b * c0;
                            const float ccp = lgg * fminf(wp, cbar);
                            const float devp = (fminf(wp, rho) * X + ccp * d) - dws;
                            const float tt = devp * devp + (ccp * ccp) * vc;
                            const float gcc = gg * c0;
                            const float dqq = ((lead + gcc * (vv1n + d)) - vv) - tb;
                            const float tq = dqq * dqq + (gcc * gcc) * vc;
                            inner = m > 0.0f ? inner + m * tt : inner;
                            innerq = m > 0.0f ? innerq + m * tq : innerq;
                        }
                        tx = inner;
                        zx = innerq;
                    }
                } else {
                    float cont = value, contq = value, below_dev = 0.0f, below_var = 0.0f, below_q = 0.0f;
                    if (CHILD) {
                        const float *below = first + (int64_t)next * F1 * n + k;
                        const float vv0n = below[0], w0n = below[n], v0n = ws[(int64_t)next * F2 * n + k];
                        cont = leaves ? value : g * vv0n;
                        contq = leaves ? value : g * w0n;
                        below_dev = leaves ? 0.0f : cc * (w0n - vv0n);
                        below_var = leaves ? 0.0f : cc2 * v0n;
                        below_q = leaves ? 0.0f : ggc2 * v0n;
                    }
                    const float dev = (cr * (base0 + g * cont) + below_dev) - d0s;
                    const float dq = ((lead0 + gc * contq) - vv) - tb;
                    tx = dev * dev + below_var;
                    zx = dq * dq + below_q;
                }
                x = live ? x + chance * tx : x;
                z = live ? z + chance * zx : z;
            }
            const bool both = mu0a > 0.0f && mu1b > 0.0f;
            acc = both ? acc + (mu0a * mu1b) * x : acc;
            const float zr = mu1b > 0.0f ? qv[a] + mu1b * z : qv[a];
            const float zc = mu0a > 0.0f ? qv[b] + mu0a * z : qv[b];
            const float vc = mu1b > 0.0f ? va[a] + mu1b * x : va[a];
            if (col_side) {
                qv[b] = zc;
                va[a] = vc;
            } else {
                qv[a] = zr;
            }
        }
    }
    float tv1 = 0.0f, qout[A], v1[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        v1[a] = mu_opp[a] > 0.0f ? va[a] : 0.0f;  // a row action never drawn conditions on nothing
        const float btw = given_row[(s * n + k) * A + a] - tgt;  // W1[a] about the column side's target
        tv1 = mu_opp[a] > 0.0f ? tv1 + mu_opp[a] * (v1[a] + btw * btw) : tv1;
        const float num = qv[a] + (1.0f - mu_own[a]) * (tbar[a] * tbar[a]);
        qout[a] = mu_own[a] > 0.0f ? num / mu_own[a] : 0.0f;
    }
    if (!on) return;
    const int64_t slot = s * n + k;
    target_var[slot * 2 + (col_side ? 1 : 0)] = col_side ? tv1 : acc;
    float *qrow = q_var + slot * (2 * A) + (col_side ? A : 0);
#pragma unroll
    for (int a = 0; a < A; ++a) qrow[a] = qout[a];
    float *mine = ws + s * F2 * n + k;
    if (col_side) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
            given_row_var[slot * A + a] = v1[a];
            mine[(1 + a) * n] = v1[a];
        }
    } else {
        mine[0] = acc;
    }
}

// One level, bottom-up.  grid = ceil(n_states / kWaves).
template <int A>
__global__ __launch_bounds__(kThreads) void k_vtrace_moments(const Trans *__restrict__ trans, int C, const int32_t *__restrict__ order,
                                                             int64_t n_states, int n, const Hyper hyper, const float *__restrict__ mu,
                                                             const float *__restrict__ pip, const float *__restrict__ lpol,
                                                             const float *__restrict__ vvs, const float *__restrict__ first,
                                                             const float *__restrict__ target, const float *__restrict__ given_row,
                                                             const float *__restrict__ q, float *__restrict__ target_var,
                                                             float *__restrict__ given_row_var, float *__restrict__ q_var, float *ws) {
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
    const int64_t slot = (int64_t)s * n + kk, row_of = slot * (2 * A);
    const float eta = hyper.eta[kk], g = hyper.gamma[kk], lam = hyper.lambda[kk], rho = hyper.rho[kk], cbar = hyper.c[kk];
    const float vv = vvs[slot * 2 + side];
    const float tgt = target[slot * 2 + side];
    float mu_own[A], mu_opp[A], cs_own[A], cs_opp[A], tbar[A];
    float e_own = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        mu_own[a] = mu[row_of + side * A + a];
        mu_opp[a] = mu[row_of + (1 - side) * A + a];
        const float pip_own = pip[row_of + side * A + a], pip_opp = pip[row_of + (1 - side) * A + a];
        const float lpol_own = lpol[row_of + side * A + a];
        e_own = pip_own > 0.0f ? e_own + pip_own * lpol_own : e_own;  // the entropy term, as k_vtrace_expect forms it: the same bits
        cs_own[a] = mu_own[a] > 0.0f ? pip_own / mu_own[a] : 0.0f;
        cs_opp[a] = mu_opp[a] > 0.0f ? pip_opp / mu_opp[a] : 0.0f;
        tbar[a] = q[row_of + side * A + a] - (vv - eta * lpol_own);  // the mean of the sampled tail, off the expected q
    }
    const float e_opp = __shfl_xor(e_own, kHalf);
    const float e0 = col_side ? e_opp : e_own, e1 = col_side ? e_own : e_opp;
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
        vtrace_moments_state<A, true>(rec, C, n, kk, on, col_side, s, eta, g, lam, rho, cbar, mu_own, mu_opp, cs_own, cs_opp, tbar, e0, e1, vv,
                                      tgt, first, given_row, target_var, given_row_var, q_var, ws);
    else
        vtrace_moments_state<A, false>(rec, C, n, kk, on, col_side, s, eta, g, lam, rho, cbar, mu_own, mu_opp, cs_own, cs_opp, tbar, e0, e1, vv,
                                       tgt, first, given_row, target_var, given_row_var, q_var, ws);
}

}  // namespace

extern "C" int64_t rnad_vtrace_moments_workspace(int64_t S, int A, int n) {
    if (S < 2 || n < 1 || n > RNAD_CROSS_PLAY_MAX || A < 1 || A > RNAD_MAX_ACTIONS) return -1;
    return S * n * moment_fields(A);
}

extern "C" int rnad_vtrace_moments(const rnad_tree_t *tree, int n, const float *hyper, const float *mu, const float *pip, const float *lpol,
                                   const float *vv, const float *expect_workspace, const float *target, const float *target_given_row,
                                   const float *q, float *target_var, float *target_given_row_var, float *q_var, float *workspace,
                                   void *stream_) {
    RNAD_REQUIRE(tree && hyper && mu && pip && lpol && vv && expect_workspace && target && target_given_row && q && target_var &&
                     target_given_row_var && q_var && workspace,
                 "rnad_vtrace_moments: null argument");
    RNAD_REQUIRE(n >= 1 && n <= RNAD_CROSS_PLAY_MAX, "rnad_vtrace_moments: %d members outside [1,%d]", n, RNAD_CROSS_PLAY_MAX);
    RNAD_REQUIRE(tree->S >= 2, "rnad_vtrace_moments: a tree of %lld states has no root", (long long)tree->S);
    Hyper h = {};
    for (int k = 0; k < RNAD_CROSS_PLAY_MAX; ++k) {
        const float *x = hyper + 5 * (k < n ? k : 0);
        h.eta[k] = x[0], h.gamma[k] = x[1], h.lambda[k] = x[2], h.rho[k] = x[3], h.c[k] = x[4];
        RNAD_REQUIRE(std::isfinite(x[0]) && std::isfinite(x[2]), "rnad_vtrace_moments: eta[%d] = %g or lambda[%d] = %g is not finite", k,
                     (double)x[0], k, (double)x[2]);
        RNAD_REQUIRE(x[1] > 0.0f && std::isfinite(x[1]), "rnad_vtrace_moments: gamma[%d] = %g is not a positive number", k, (double)x[1]);
        RNAD_REQUIRE(x[3] >= 0.0f && x[4] >= 0.0f, "rnad_vtrace_moments: the clips rho[%d] = %g, c[%d] = %g must not be negative", k,
                     (double)x[3], k, (double)x[4]);
    }
    RNAD_REQUIRE(tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS && tree->trans &&
                     tree->level_order && tree->order_pos && tree->n_levels >= 1 &&
                     tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_vtrace_moments: bad tree");
    {  // no output may overlap an input (the first moments and their export record included) or another output anywhere
        const size_t column = (size_t)tree->S * (size_t)n * sizeof(float), A = (size_t)tree->A, table = column * 2 * A;
        constexpr int kIn = 8, kAll = 12;
        const struct { const char *p; size_t n; } buf[kAll] = {
            {(const char *)mu, table},
            {(const char *)pip, table},
            {(const char *)lpol, table},
            {(const char *)vv, column * 2},
            {(const char *)target, column * 2},
            {(const char *)target_given_row, column * A},
            {(const char *)q, table},
            {(const char *)expect_workspace, column * (size_t)first_fields(tree->A)},
            {(const char *)target_var, column * 2},
            {(const char *)target_given_row_var, column * A},
            {(const char *)q_var, table},
            {(const char *)workspace, column * (size_t)moment_fields(tree->A)}};
        for (int j = kIn; j < kAll; ++j)
            RNAD_REQUIRE(buf[kIn - 1].p + buf[kIn - 1].n <= buf[j].p || buf[j].p + buf[j].n <= buf[kIn - 1].p,
                         "rnad_vtrace_moments: expect_workspace overlaps an output");
        for (int i = 0; i < kAll; ++i)
            for (int j = (i < kIn ? kIn : i + 1); j < kAll; ++j)
                RNAD_REQUIRE(buf[i].p + buf[i].n <= buf[j].p || buf[j].p + buf[j].n <= buf[i].p,
                             i < kIn ? "rnad_vtrace_moments: an output overlaps an input" : "rnad_vtrace_moments: two outputs overlap");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_vtrace_moments: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_vtrace_moments_init, dim3((unsigned)((tree->S + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       tree->order_pos, tree->S, tree->A, n, target_var, target_given_row_var, q_var, workspace);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_vtrace_moments<kA>), dim3((unsigned)((cnt + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream,
                                   tree->trans, tree->C, tree->level_order + off, cnt, n, h, mu, pip, lpol, vv, expect_workspace, target,
                                   target_given_row, q, target_var, target_given_row_var, q_var, workspace);
        }
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
