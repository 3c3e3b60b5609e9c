// replay.hip -- the fast records of a REPLAYED compact batch: the on-policy table of this step with its two acting-policy column blocks
// rebuilt from the policy rows the batch was played with (rnad_bucket_behaviour_records, include/rnad_hip.h).
//
// fast_slot (bucket.hip) reads the acting policy of a slot in two places of its row's fast record, cs[act] = pi_processed / mu and
// inv_mu[act] = 1 / mu (_policy_ratio, learn/vtrace.py:199-204); write_row_records (row_records.hpp) fills both with the actor's own pi
// standing in for mu.  With mu = the stored rows of an older net the very same learner is the off-policy one.  The divisions are the
// IEEE fp32 ones write_row_records makes (same build flags), so a behaviour that IS the actor gives the on-policy table bit for bit.
#include "common.hpp"
#include "row_records.hpp"

namespace rnad {
namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 64;  // rows of the tables a workgroup converts: 64 * (A + 1) 16-byte pieces of the record, 9 KB of LDS at A = 8

// the tables of up to RNAD_BEHAVIOUR_MAX behaviours, by value in the kernel arguments (a captured launch keeps them)
struct BehaviourTables {
    const float *mu[RNAD_BEHAVIOUR_MAX];
    float *out[RNAD_BEHAVIOUR_MAX];
};

// One workgroup per kTileRows rows (of the row list, when there is one).  The tile's on-policy records are read ONCE, as 16-byte pieces
// with the lanes of a wave on consecutive pieces, and kept in LDS; per behaviour its policy rows are staged the same way and every
// thread rebuilds one 16-byte piece of an output record, which leaves as one 16-byte store -- consecutive lanes, consecutive pieces (a
// store per float would touch 64 different records per instruction: row_records.hpp).
template <int A>
__global__ __launch_bounds__(kThreads) void k_behaviour_records(int64_t rows, int n, const float *__restrict__ fast, BehaviourTables tabs,
                                                                 const int32_t *__restrict__ row_list, const int64_t *__restrict__ n_rows) {
    constexpr int F = dev::kFastStride<A>, F4 = F / 4;      // floats / 16-byte pieces of a fast record
    constexpr int P = dev::kPolStride<A>, P4 = P / 4;       // ... of a policy row
    constexpr int kCs = 4 + 2 * A, kInv = 4 + 3 * A;        // first float of the cs and of the inv_mu block
    __shared__ float4 s_rec[kTileRows * F4];
    __shared__ float4 s_mu[kTileRows * P4];
    __shared__ int32_t s_row[kTileRows];
    const int64_t count = row_list ? *n_rows : rows;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
    if (row0 >= count) return;  // (the whole workgroup)
    const int tile = (int)(count - row0 < kTileRows ? count - row0 : kTileRows);
    const int tid = threadIdx.x;
    if (tid < tile) s_row[tid] = row_list ? row_list[row0 + tid] : (int32_t)(row0 + tid);
    __syncthreads();
    const float4 *fast4 = reinterpret_cast<const float4 *>(fast);
    for (int g = tid; g < tile * F4; g += kThreads) {
        const int i = g / F4, p = g - i * F4;
        s_rec[g] = fast4[(int64_t)s_row[i] * F4 + p];
    }
    const float *rec_f = reinterpret_cast<const float *>(s_rec);
    const float *mu_f = reinterpret_cast<const float *>(s_mu);
#pragma unroll
    for (int k = 0; k < RNAD_BEHAVIOUR_MAX; ++k) {
        if (k >= n) break;  // (uniform)
        __syncthreads();    // the records are staged; the last behaviour's rows have been read
        const float4 *mu4 = reinterpret_cast<const float4 *>(tabs.mu[k]);
        for (int g = tid; g < tile * P4; g += kThreads) {
            const int i = g / P4, p = g - i * P4;
            s_mu[g] = mu4[(int64_t)s_row[i] * P4 + p];
        }
        __syncthreads();
        float4 *out4 = reinterpret_cast<float4 *>(tabs.out[k]);
        for (int g = tid; g < tile * F4; g += kThreads) {
            const int i = g / F4, p = g - i * F4;
            const float4 in = s_rec[g];
            float o[4] = {in.x, in.y, in.z, in.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = 4 * p + u;
                if (j >= kCs) {  // cs[a] = pi_processed[a] / mu[a], inv_mu[a] = 1 / mu[a]: write_row_records' two divisions
                    const bool inv = j >= kInv;
                    const int a = j - (inv ? kInv : kCs);
                    const float num = inv ? 1.0f : rec_f[i * F + 4 + a];
                    o[u] = num / mu_f[i * P + a];
                }
            }
            out4[(int64_t)s_row[i] * F4 + p] = float4{o[0], o[1], o[2], o[3]};
        }
    }
}

bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace
}  // namespace rnad

using namespace rnad;

extern "C" int rnad_bucket_behaviour_records(const rnad_tree_t *tree, int n, const float *fast_records, const float *const *mu_rows,
                                             float *const *out, const int32_t *rows, const int64_t *n_rows, void *stream) {
    RNAD_REQUIRE(n >= 1 && n <= RNAD_BEHAVIOUR_MAX, "rnad_bucket_behaviour_records: n = %d behaviours outside 1 .. %d", n, RNAD_BEHAVIOUR_MAX);
    RNAD_REQUIRE(tree && fast_records && mu_rows && out, "rnad_bucket_behaviour_records: null argument");
    RNAD_REQUIRE(!rows == !n_rows, "rnad_bucket_behaviour_records: rows and n_rows go together");
    const int A = tree->A;
    RNAD_REQUIRE(A >= 1 && A <= RNAD_MAX_ACTIONS, "max_actions %d out of range [1,%d]", A, RNAD_MAX_ACTIONS);
    const int64_t N = 2 * tree->S;
    const size_t rec_bytes = (size_t)N * (size_t)(4 + 4 * A) * sizeof(float), mu_bytes = (size_t)N * (size_t)((A + 3) & ~3) * sizeof(float);
    BehaviourTables tabs{};
    for (int k = 0; k < n; ++k) {
        RNAD_REQUIRE(mu_rows[k] && out[k], "rnad_bucket_behaviour_records: null table of behaviour %d", k);
        tabs.mu[k] = mu_rows[k];
        tabs.out[k] = out[k];
    }
    RNAD_REQUIRE(((uintptr_t)fast_records & 15) == 0, "rnad_bucket_behaviour_records: fast_records must be 16-byte aligned");
    for (int k = 0; k < n; ++k)
        RNAD_REQUIRE(((uintptr_t)mu_rows[k] & 15) == 0 && ((uintptr_t)out[k] & 15) == 0,
                     "rnad_bucket_behaviour_records: the tables of behaviour %d must be 16-byte aligned", k);
    for (int k = 0; k < n; ++k) {
        RNAD_REQUIRE(!overlap(out[k], rec_bytes, fast_records, rec_bytes), "rnad_bucket_behaviour_records: out[%d] overlaps fast_records", k);
        for (int j = 0; j < n; ++j) {
            RNAD_REQUIRE(!overlap(out[k], rec_bytes, mu_rows[j], mu_bytes), "rnad_bucket_behaviour_records: out[%d] overlaps mu_rows[%d]", k, j);
            RNAD_REQUIRE(j == k || !overlap(out[k], rec_bytes, out[j], rec_bytes), "rnad_bucket_behaviour_records: out[%d] overlaps out[%d]", k, j);
        }
    }
    if (N == 0) return 0;
    const unsigned blocks = (unsigned)((N + kTileRows - 1) / kTileRows);
    RNAD_DISPATCH_A(A, hipLaunchKernelGGL((k_behaviour_records<kA>), dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, N, n, fast_records,
                                          tabs, rows, n_rows));
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
