// reg_solve.hip -- exact tabular R-NaD: the fixed point of one regularisation update on the whole tree, one bottom-up sweep (gfx950).
//
// Sits next to: cross_play.hip and the bottom-up half of nashconv.hip, and walks the same tables.  Every reachable state is a matrix game
//   Q[s,r,c] = sum_t chance[s,t,r,c] * (next == 0 ? value[s,t,r,c] : V[next])                 (entries with chance <= 0 skipped)
// and the sweep finds its equilibrium with the KL terms of learn/vtrace.py:234-239 added (mu: the regularisation policy, eta > 0):
//   pi_row ~ mu_row * exp((Q pi_col) / eta)        pi_col ~ mu_col * exp(-(Q^T pi_row) / eta)
//   V[s] = pi_row^T Q pi_col - eta * KL(pi_row || mu_row) + eta * KL(pi_col || mu_col)
// V is the row player's regularised value (the sign of player_others, vtrace.py:237).  That game is strongly monotone, so the pair is
// unique, and the children's V are finished when a level starts: backward induction over level_order.  Citations are baskuit/R-NaD file:line.
//
// Work split: one lane per state, as in nashconv.hip.  The lane builds Q (A * A floats) from its records once and then iterates in
// registers on l = log pi -- after a few updates log mu lies below -500, which only a log representation survives:
//   step(l, q) = x - logsumexp(x),  x = (l + tau * eta * log mu + tau * q) / (1 + tau * eta)       (magnet mirror descent)
//   l_half = step(l, q(l));   l <- step(l, q(l_half))                                              (extragradient: q at the half step)
// with tau = 1 / (2 max|Q|) and q = (Q pi_col, -Q^T pi_row).  The state stops when its residual, max_a |pi(a) - softmax(log mu + q / eta)(a)|
// over both players -- in probability space: a log-space residual is ruled by actions of probability e^-20 -- is <= tol, or after
// max_iters steps.  An action that is illegal or has mu = 0 is outside the support: pi = 0, log pi = -inf, and it enters no product.
#include "common.hpp"

#include <cmath>

using namespace rnad;

namespace {

// One wave per workgroup.  A wave runs until its slowest state is done, so nothing is shared inside a workgroup that a larger one would
// save.  Measured against 256 threads (profiles/tabular_rnad.md): medians of the first pair of runs, 0.753 against 0.790 ms on the configs[1]
// tree and 6.021 against 5.983 ms on the configs[3]-shaped one -- no case for the larger workgroup.
constexpr int kThreads = 64;
inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// Rows the sweep never reaches -- the absorbing state 0 and states no chance > 0 path leads to: zeros, log_policy -inf.  A kernel, not a
// memset node (zero_async in common.hpp); it runs first, so V[0] = 0 is in place when a record without a child selects row 0.
__global__ __launch_bounds__(256) void k_reg_solve_zero(const int32_t *__restrict__ order_pos, int64_t S, int A2, float *__restrict__ log_policy,
                                                        float *__restrict__ policy, float *__restrict__ values, float *__restrict__ residual,
                                                        int32_t *__restrict__ iters) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= S || order_pos[s] >= 0) return;
    for (int a = 0; a < A2; ++a) {
        log_policy[s * A2 + a] = -INFINITY;
        policy[s * A2 + a] = 0.0f;
    }
    values[s] = 0.0f;
    residual[s] = 0.0f;
    iters[s] = 0;
}

// x - logsumexp(x) over the support; entries outside it stay 0 and are never read as logs.
template <int A>
__device__ __forceinline__ void normalise(float (&x)[A], unsigned on) {
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < A; ++a) m = ((on >> a) & 1) && x[a] > m ? x[a] : m;
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) sum += ((on >> a) & 1) ? expf(x[a] - m) : 0.0f;
    const float lse = m + logf(sum);
#pragma unroll
    for (int a = 0; a < A; ++a) x[a] = ((on >> a) & 1) ? x[a] - lse : 0.0f;
}

template <int A>
__device__ __forceinline__ void probabilities(const float (&l)[A], unsigned on, float (&p)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) p[a] = ((on >> a) & 1) ? expf(l[a]) : 0.0f;
}

// q of both players against the other's policy: qr = Q pc, qc = -(Q^T pr); c inside r, a fixed order.
template <int A>
__device__ __forceinline__ void responses(const float (&Q)[A * A], const float (&pr)[A], const float (&pc)[A], float (&qr)[A], float (&qc)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) qr[a] = qc[a] = 0.0f;
#pragma unroll
    for (int r = 0; r < A; ++r) {
#pragma unroll
        for (int c = 0; c < A; ++c) {
            qr[r] += Q[r * A + c] * pc[c];
            qc[c] -= pr[r] * Q[r * A + c];
        }
    }
}

// max_a |p(a) - softmax(lm + q / eta)(a)| over the support of one player
template <int A>
__device__ __forceinline__ float residual_of(const float (&p)[A], const float (&lm)[A], const float (&q)[A], unsigned on, float inv_eta) {
    float t[A];
#pragma unroll
    for (int a = 0; a < A; ++a) t[a] = lm[a] + q[a] * inv_eta;
    float m = -INFINITY;
#pragma unroll
    for (int a = 0; a < A; ++a) m = ((on >> a) & 1) && t[a] > m ? t[a] : m;
    float sum = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        t[a] = ((on >> a) & 1) ? expf(t[a] - m) : 0.0f;
        sum += t[a];
    }
    float res = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float d = fabsf(p[a] - t[a] / sum);
        res = ((on >> a) & 1) && d > res ? d : res;
    }
    return res;
}

template <int A>
__device__ __forceinline__ void step(const float (&l)[A], const float (&lm)[A], const float (&q)[A], unsigned on, float tau, float tau_eta,
                                     float inv_1p, float (&out)[A]) {
#pragma unroll
    for (int a = 0; a < A; ++a) out[a] = (l[a] + tau_eta * lm[a] + tau * q[a]) * inv_1p;
    normalise<A>(out, on);
}

// One level: the regularised equilibrium of each of its states from the finished values below it.
template <int A>
__global__ __launch_bounds__(kThreads) void k_reg_solve(const Trans *__restrict__ trans, const float *__restrict__ node, int C,
                                                        const int32_t *__restrict__ order, int64_t n, float eta, float tol, int max_iters,
                                                        const float *__restrict__ log_reg, float *__restrict__ log_policy,
                                                        float *__restrict__ policy, float *values, float *__restrict__ residual,
                                                        int32_t *__restrict__ iters) {
    constexpr int AA = A * A, NS = (AA + 2 + 3) & ~3;
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const int s = order[k];
    const Trans *e = trans + (int64_t)s * AA * C;
    const float *nd = node + (int64_t)s * NS;
    const uint64_t bits = (uint64_t)__float_as_uint(nd[AA]) | ((uint64_t)__float_as_uint(nd[AA + 1]) << 32);

    // the matrix game: per joint action the chance outcomes in order, one accumulator (as cross_play_state); the records are read here only
    float Q[AA];
#pragma unroll
    for (int rc = 0; rc < AA; ++rc) Q[rc] = 0.0f;
    for (int t = 0; t < C; ++t) {
#pragma unroll
        for (int rc = 0; rc < AA; ++rc) {
            const Trans x = e[rc * C + t];
            const bool live = x.chance > 0.0f;
            const int next = live ? x.next : 0;
            const float child = values[next];  // row 0 holds 0 (k_reg_solve_zero) and is discarded
            const float v = next == 0 ? x.value : child;
            Q[rc] = live ? Q[rc] + x.chance * v : Q[rc];
        }
    }
    float max_q = 0.0f;
#pragma unroll
    for (int rc = 0; rc < AA; ++rc) max_q = fmaxf(max_q, fabsf(Q[rc]));

    // supports and magnets; an entry outside the support holds 0 and is masked wherever it could matter
    const float *reg = log_reg + (int64_t)s * 2 * A;
    unsigned on_r = 0, on_c = 0;
    float mr[A], mc[A], lr[A], lc[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
        const float xr = reg[a], xc = reg[A + a];
        const bool r_on = ((bits >> (a * A)) & 1) && xr > -INFINITY;  // legal_tensor[s, 0, :, 0]
        const bool c_on = ((bits >> a) & 1) && xc > -INFINITY;        // legal_tensor[s, 0, 0, :]
        on_r |= (unsigned)r_on << a;
        on_c |= (unsigned)c_on << a;
        lr[a] = mr[a] = r_on ? xr : 0.0f;
        lc[a] = mc[a] = c_on ? xc : 0.0f;
    }
    normalise<A>(lr, on_r);  // the iterate starts at the magnet
    normalise<A>(lc, on_c);

    const float inv_eta = 1.0f / eta;
    const float tau = 0.5f / fmaxf(max_q, 1e-6f), tau_eta = tau * eta, inv_1p = 1.0f / (1.0f + tau_eta);
    float pr[A], pc[A], qr[A], qc[A];
    float res;
    int it = 0;
    for (;;) {
        probabilities<A>(lr, on_r, pr);
        probabilities<A>(lc, on_c, pc);
        responses<A>(Q, pr, pc, qr, qc);
        res = fmaxf(residual_of<A>(pr, mr, qr, on_r, inv_eta), residual_of<A>(pc, mc, qc, on_c, inv_eta));
        if (res <= tol || it >= max_iters) break;
        float hr[A], hc[A], ph_r[A], ph_c[A], qhr[A], qhc[A];
        step<A>(lr, mr, qr, on_r, tau, tau_eta, inv_1p, hr);
        step<A>(lc, mc, qc, on_c, tau, tau_eta, inv_1p, hc);
        probabilities<A>(hr, on_r, ph_r);
        probabilities<A>(hc, on_c, ph_c);
        responses<A>(Q, ph_r, ph_c, qhr, qhc);
        step<A>(lr, mr, qhr, on_r, tau, tau_eta, inv_1p, hr);
        step<A>(lc, mc, qhc, on_c, tau, tau_eta, inv_1p, hc);
#pragma unroll
        for (int a = 0; a < A; ++a) {
            lr[a] = hr[a];
            lc[a] = hc[a];
        }
        ++it;
    }

    // V from the last evaluation: pi_row^T (Q pi_col), then the two KL sums, each in action order
    float game = 0.0f, kl_r = 0.0f, kl_c = 0.0f;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        game += pr[a] * qr[a];
        kl_r += pr[a] * (lr[a] - mr[a]);
        kl_c += pc[a] * (lc[a] - mc[a]);
    }
    float *lp = log_policy + (int64_t)s * 2 * A, *pp = policy + (int64_t)s * 2 * A;
#pragma unroll
    for (int a = 0; a < A; ++a) {
        lp[a] = ((on_r >> a) & 1) ? lr[a] : -INFINITY;
        lp[A + a] = ((on_c >> a) & 1) ? lc[a] : -INFINITY;
        pp[a] = pr[a];
        pp[A + a] = pc[a];
    }
    values[s] = game - eta * kl_r + eta * kl_c;
    residual[s] = res;
    iters[s] = it;
}

}  // namespace

extern "C" int rnad_reg_solve(const rnad_tree_t *tree, float eta, float tol, int max_iters, const float *log_reg, float *log_policy,
                              float *policy, float *values, float *residual, int32_t *iters, void *stream_) {
    RNAD_REQUIRE(eta > 0.0f && std::isfinite(eta), "rnad_reg_solve: eta %g is not a positive number (the unregularised game has no unique fixed point)",
                 (double)eta);
    RNAD_REQUIRE(tol > 0.0f && std::isfinite(tol), "rnad_reg_solve: tol %g is not a positive number", (double)tol);
    RNAD_REQUIRE(max_iters >= 1, "rnad_reg_solve: max_iters %d below 1", max_iters);
    RNAD_REQUIRE(tree && log_reg && log_policy && policy && values && residual && iters, "rnad_reg_solve: null argument");
    RNAD_REQUIRE((const void *)log_policy != (const void *)log_reg && (const void *)policy != (const void *)log_reg &&
                     (const void *)values != (const void *)log_reg && (const void *)residual != (const void *)log_reg &&
                     (const void *)iters != (const void *)log_reg,
                 "rnad_reg_solve: an output aliases log_reg");
    RNAD_REQUIRE(tree->S >= 2 && tree->A >= 1 && tree->A <= RNAD_MAX_ACTIONS && tree->C >= 1 && tree->C <= RNAD_MAX_TRANSITIONS &&
                     tree->trans && tree->node && tree->level_order && tree->order_pos && tree->n_levels >= 1 &&
                     tree->level_offsets.size() == (size_t)tree->n_levels + 1,
                 "rnad_reg_solve: bad tree");
    {  // with the sizes known: no output may overlap log_reg or another output anywhere, not only at its first byte
        const size_t table = (size_t)tree->S * 2 * (size_t)tree->A * sizeof(float), column = (size_t)tree->S * sizeof(float);
        const struct { const char *p; size_t n; } buf[6] = {{(const char *)log_reg, table},  {(const char *)log_policy, table}, {(const char *)policy, table},
                                                             {(const char *)values, column},  {(const char *)residual, column},  {(const char *)iters, column}};
        for (int i = 0; i < 6; ++i)
            for (int j = i + 1; j < 6; ++j)
                RNAD_REQUIRE(buf[i].p + buf[i].n <= buf[j].p || buf[j].p + buf[j].n <= buf[i].p,
                             i == 0 ? "rnad_reg_solve: an output aliases log_reg (it overlaps it)" : "rnad_reg_solve: two outputs overlap");
    }
    hipStream_t stream = (hipStream_t)stream_;
    DeviceGuard guard(tree->device);
    RNAD_REQUIRE(guard.ok, "rnad_reg_solve: cannot select device %d", tree->device);
    hipLaunchKernelGGL(k_reg_solve_zero, dim3((unsigned)((tree->S + 255) / 256)), dim3(256), 0, stream, tree->order_pos, tree->S, 2 * tree->A,
                       log_policy, policy, values, residual, iters);
    RNAD_DISPATCH_A(tree->A, {
        for (int l = tree->n_levels - 1; l >= 0; --l) {
            const int64_t off = tree->level_offsets[l], cnt = tree->level_offsets[l + 1] - off;
            if (cnt > 0)
                hipLaunchKernelGGL((k_reg_solve<kA>), dim3(blocks_for(cnt)), dim3(kThreads), 0, stream, tree->trans, tree->node, tree->C,
                                   tree->level_order + off, cnt, eta, tol, max_iters, log_reg, log_policy, policy, values, residual, iters);
        }
    });
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
