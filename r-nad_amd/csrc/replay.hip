// replay.hip -- the fast records of a REPLAYED compact batch: the on-policy table of this step with its two acting-policy column blocks
// rebuilt from the policy rows the batch was played with (rnad_bucket_behaviour_records, include/rnad_hip.h).
//
// fast_slot (bucket.hip) reads the acting policy of a slot in two places of its row's fast record, cs[act] = pi_processed / mu and
// inv_mu[act] = 1 / mu (_policy_ratio, learn/vtrace.py:199-204); write_row_records (row_records.hpp) fills both with the actor's own pi
// standing in for mu.  With mu = the stored rows of an older net the very same learner is the off-policy one.  The divisions are the
// IEEE fp32 ones write_row_records makes (same build flags), so a behaviour that IS the actor gives the on-policy table bit for bit.
//
// Second half: the lane draw of a replay step (rnad_bucket_draw_lanes) -- lanes drawn across stored compact batches, compacted into one.
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

// ---------------------------------------------------------------------------------------- the lane draw (rnad_bucket_draw_lanes)
// B lanes drawn across up to RNAD_DRAW_MAX stored compact batches, compacted into ONE bucket-ordered compact batch: the drawn columns of
// source k, in their source order, in columns [off_k, off_k + b_k) of the destination, with a work list of its own per source.  A column's
// relative states depend on its bucket alone (include/rnad_hip.h), a source's columns are sorted by bucket and the compaction is stable,
// so each stretch stays sorted by bucket and the bytes of a column are copied as they are.
//
//   k_draw_count   one workgroup per (source, source item): the membership test of rnad_rng.h once per column, kept as ballot words;
//                  the item's number of drawn columns and of their live slots per parity
//   k_draw_scan    one workgroup per source: prefix of the items' counts = where each item's drawn columns go; the drawn lanes per bucket,
//                  repacked into items of at most `chunk` lanes (bucket.hip's items_phase on the drawn totals)
//   k_draw_gather  one workgroup per (source, source item): rank inside the item from the ballot words, the column's bytes copied;
//                  consecutive drawn lanes of an item land on consecutive columns
// No atomics on global memory, nothing but integers until the live-slot counts are written out as f64.
struct DrawItem {
    int32_t begin, count, bucket, single;  // bucket.hip's Item
};
struct DrawSources {
    const void *states[RNAD_DRAW_MAX];
    const uint64_t *acts[RNAD_DRAW_MAX];
    const float *final_reward[RNAD_DRAW_MAX];
    const int32_t *lane_ids[RNAD_DRAW_MAX];
    const DrawItem *items[RNAD_DRAW_MAX];
    const int32_t *n_items[RNAD_DRAW_MAX];
    DrawItem *items_out[RNAD_DRAW_MAX];
    int32_t *n_items_out[RNAD_DRAW_MAX];
    int32_t b[RNAD_DRAW_MAX], off[RNAD_DRAW_MAX];  // draw size, first destination column
};
// the caller's workspace: everything the three launches hand to each other
struct DrawWork {
    int32_t *sel;              // [RNAD_DRAW_MAX][max_items] drawn columns of a source item
    int32_t *live;             // [RNAD_DRAW_MAX][max_items][2] their live slots per parity
    int32_t *dst;              // [RNAD_DRAW_MAX][max_items] first destination column of a source item
    unsigned long long *mask;  // [RNAD_DRAW_MAX][max_items][words] membership of the item's columns, 64 per word
    unsigned long long *part;  // [RNAD_DRAW_MAX][2] live slots per source
    int64_t bytes;
};
DrawWork carve_draw(void *base, int64_t max_items, int words) {
    DrawWork w;
    uintptr_t at = (uintptr_t)base;
    auto take = [&](size_t bytes) {
        const uintptr_t here = at;
        at += (bytes + 15) & ~(size_t)15;
        return here;
    };
    w.mask = (unsigned long long *)take(sizeof(unsigned long long) * RNAD_DRAW_MAX * (size_t)max_items * (size_t)words);
    w.part = (unsigned long long *)take(sizeof(unsigned long long) * RNAD_DRAW_MAX * 2);
    w.sel = (int32_t *)take(sizeof(int32_t) * RNAD_DRAW_MAX * (size_t)max_items);
    w.live = (int32_t *)take(sizeof(int32_t) * RNAD_DRAW_MAX * (size_t)max_items * 2);
    w.dst = (int32_t *)take(sizeof(int32_t) * RNAD_DRAW_MAX * (size_t)max_items);
    w.bytes = (int64_t)(at - (uintptr_t)base);
    return w;
}

constexpr int kScanThreads = 1024;

// the lanes of a source item that the draw looks at: none of an item that does not lie inside the batch and the plan (a work list is
// device memory that the host cannot check; nothing is read or written out of bounds on its word)
__device__ __forceinline__ int draw_item_lanes(const DrawItem &item, int64_t B, int n_buckets, int words) {
    if (item.begin < 0 || item.count < 0 || (int64_t)item.begin + item.count > B || (unsigned)item.bucket >= (unsigned)n_buckets) return 0;
    return min(item.count, words * 64);
}
__device__ __forceinline__ int draw_shared_steps(const DrawItem &item, const int32_t *__restrict__ bucket_path, int n_groups, int shared_root) {
    const int path_word = bucket_path[item.bucket];
    return (path_word & (shared_root - 1)) + ((item.bucket < n_groups && (path_word & shared_root)) ? 2 : 0);
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename REL>
__global__ __launch_bounds__(kThreads) void k_draw_count(DrawSources src, int T_cap, int64_t B, uint64_t seed, int source0, int n_groups, int n_buckets,
                                                          int shared_root, const int32_t *__restrict__ bucket_path, int words, int64_t max_items,
                                                          DrawWork w) {
    const int k = blockIdx.y, i = blockIdx.x;
    if (i >= *src.n_items[k]) return;  // (the whole workgroup)
    const DrawItem item = src.items[k][i];
    const int lanes = draw_item_lanes(item, B, n_buckets, words);
    const int n_shared = lanes ? draw_shared_steps(item, bucket_path, n_groups, shared_root) : 0;
    const REL *__restrict__ states = static_cast<const REL *>(src.states[k]);
    const int64_t bk = src.b[k];
    __shared__ int s_sum[3];
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int64_t slot = (int64_t)k * max_items + i;
    int sel_n = 0, live0 = 0, live1 = 0;
    for (int base = 0; base < words * 64; base += kThreads) {  // (uniform)
        const int l = base + (int)threadIdx.x;
        const int64_t j = (int64_t)item.begin + l;
        const bool sel = l < lanes && rnad_draw_selected(seed, (uint32_t)(source0 + k), B, bk, j) != 0;
        const unsigned long long m = __ballot(sel);
        if ((threadIdx.x & 63) == 0 && (l >> 6) < words) w.mask[slot * words + (l >> 6)] = m;
        if (sel) {
            sel_n += 1;
            for (int t = 0; t < T_cap; ++t) {
                const int live = t < n_shared ? 1 : (states[(int64_t)t * B + j] != 0 ? 1 : 0);
                if (t & 1) live1 += live;
                else live0 += live;
            }
        }
    }
    sel_n = wave_sum(sel_n);
    live0 = wave_sum(live0);
    live1 = wave_sum(live1);
    if ((threadIdx.x & 63) == 0) {  // (LDS integer adds: four waves)
        atomicAdd(&s_sum[0], sel_n);
        atomicAdd(&s_sum[1], live0);
        atomicAdd(&s_sum[2], live1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        w.sel[slot] = s_sum[0];
        w.live[2 * slot] = s_sum[1];
        w.live[2 * slot + 1] = s_sum[2];
    }
}

// inclusive prefix of v over the workgroup (kScanThreads threads); wave_s: 16 words of LDS.  Ends on a barrier: wave_s may be reused.
__device__ __forceinline__ int block_scan(int v, int32_t *wave_s) {
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(s, off, 64);
        if ((int)(threadIdx.x & 63) >= off) s += a;
    }
    if ((threadIdx.x & 63) == 63) wave_s[threadIdx.x >> 6] = s;
    __syncthreads();
    for (int x = 0; x < (int)(threadIdx.x >> 6); ++x) s += wave_s[x];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(kScanThreads) void k_draw_scan(DrawSources src, int n_buckets, int chunk, int64_t max_items, int sole, DrawWork w) {
    extern __shared__ int32_t lds[];
    int32_t *start_s = lds, *first_s = lds + n_buckets + 1;  // [n_buckets + 1] each: first drawn lane / first new item of a bucket
    __shared__ int32_t wave_s[16];
    __shared__ int32_t carry_s;
    __shared__ unsigned long long live_s[2];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int n_src = (int)min((int64_t)*src.n_items[k], max_items);
    const DrawItem *__restrict__ items = src.items[k];
    for (int b = tid; b <= n_buckets; b += kScanThreads) start_s[b] = first_s[b] = 0;
    if (tid == 0) carry_s = 0;
    if (tid < 2) live_s[tid] = 0;
    __syncthreads();
    // 1. the source items in order: where the drawn columns of each go; first and last drawn lane of every bucket (a bucket's source
    //    items are consecutive), kept as [start, end) in start_s / first_s
    unsigned long long live0 = 0, live1 = 0;
    for (int base = 0; base < n_src; base += kScanThreads) {
        const int i = base + tid;
        const bool in = i < n_src;
        const int64_t slot = (int64_t)k * max_items + i;
        const int c = in ? w.sel[slot] : 0;
        const int incl = block_scan(c, wave_s);
        const int pre = carry_s + incl - c;
        if (in) {
            live0 += (unsigned)w.live[2 * slot];
            live1 += (unsigned)w.live[2 * slot + 1];
            w.dst[slot] = src.off[k] + pre;
            const int bucket = items[i].bucket;
            if ((unsigned)bucket < (unsigned)n_buckets) {
                if (i == 0 || items[i - 1].bucket != bucket) start_s[bucket] = pre;
                if (i + 1 == n_src || items[i + 1].bucket != bucket) first_s[bucket] = pre + c;
            }
        }
        __syncthreads();  // (every thread has read carry_s)
        if (tid == kScanThreads - 1) carry_s += incl;
        __syncthreads();
    }
    atomicAdd(&live_s[0], live0);  // (LDS, integers)
    atomicAdd(&live_s[1], live1);
    // 2. a thread takes `per` consecutive buckets: drawn lanes and new items of each, one scan of either over the workgroup
    const int per = (n_buckets + kScanThreads - 1) / kScanThreads;
    const int b0 = min(n_buckets, tid * per), b1 = min(n_buckets, b0 + per);
    int own_l = 0, own_i = 0;
    for (int b = b0; b < b1; ++b) {
        const int n = max(first_s[b] - start_s[b], 0);
        own_l += n;
        own_i += (n + chunk - 1) / chunk;
    }
    int run_l = block_scan(own_l, wave_s) - own_l, run_i = block_scan(own_i, wave_s) - own_i;
    for (int b = b0; b < b1; ++b) {
        const int n = max(first_s[b] - start_s[b], 0);
        start_s[b] = run_l;
        first_s[b] = run_i;
        run_l += n;
        run_i += (n + chunk - 1) / chunk;
    }
    if (tid == kScanThreads - 1) {  // (its buckets are the last ones, or none)
        start_s[n_buckets] = run_l;
        first_s[n_buckets] = run_i;
    }
    __syncthreads();
    // 3. the new items: item o belongs to the bucket b with first_s[b] <= o < first_s[b + 1]
    const int total = (int)min((int64_t)first_s[n_buckets], max_items);
    if (tid == 0) {
        *src.n_items_out[k] = total;
        w.part[2 * k] = live_s[0];
        w.part[2 * k + 1] = live_s[1];
    }
    DrawItem *__restrict__ out = src.items_out[k];
    for (int o = tid; o < total; o += kScanThreads) {
        int b = 0, hi = n_buckets;  // first_s[b] <= o < first_s[hi] throughout (first_s[0] = 0, first_s[n_buckets] > o)
        while (b + 1 < hi) {
            const int mid = (b + hi) >> 1;
            if (first_s[mid] <= o) b = mid;
            else hi = mid;
        }
        const int c = o - first_s[b], n = start_s[b + 1] - start_s[b];
        out[o] = DrawItem{src.off[k] + start_s[b] + c * chunk, min(chunk, n - c * chunk), b, (sole && first_s[b + 1] - first_s[b] == 1) ? 1 : 0};
    }
}

struct DrawOut {
    void *states;
    uint64_t *acts;
    float *final_reward;
    int32_t *lane_ids;
    double *norm;
};

template <typename REL>
__global__ __launch_bounds__(kThreads) void k_draw_gather(DrawSources src, int n, int T1, int64_t B, int64_t offset, int n_groups, int n_buckets,
                                                           int shared_root, const int32_t *__restrict__ bucket_path, int words, int64_t max_items,
                                                           DrawWork w, DrawOut out) {
    const int k = blockIdx.y, i = blockIdx.x;
    if (i == 0 && k == 0 && threadIdx.x < 2) {  // the live slots of the draw so far: integers, exact in f64 in any order
        unsigned long long sum = 0;
        for (int s = 0; s < n; ++s) sum += w.part[2 * s + threadIdx.x];
        out.norm[threadIdx.x] = (offset == 0 ? 0.0 : out.norm[threadIdx.x]) + (double)sum;
    }
    if (i >= *src.n_items[k]) return;  // (the whole workgroup)
    const DrawItem item = src.items[k][i];
    const int lanes = draw_item_lanes(item, B, n_buckets, words);
    if (lanes == 0) return;
    const int64_t slot = (int64_t)k * max_items + i;
    if (w.sel[slot] == 0) return;
    // rows t < n_shared of a column are neither written nor read: the bucket's own path states
    const int t0 = min(draw_shared_steps(item, bucket_path, n_groups, shared_root), T1);
    const REL *__restrict__ from = static_cast<const REL *>(src.states[k]);
    REL *__restrict__ to = static_cast<REL *>(out.states);
    const unsigned long long *__restrict__ mask = w.mask + slot * words;
    const int64_t d0 = w.dst[slot];
    for (int base = 0; base < lanes; base += kThreads) {
        const int l = base + (int)threadIdx.x;
        if (l >= lanes) break;
        const int word = l >> 6, bit = l & 63;
        const unsigned long long m = mask[word];
        if (!((m >> bit) & 1ull)) continue;
        int rank = __popcll(m & ((1ull << bit) - 1ull));
        for (int x = 0; x < word; ++x) rank += __popcll(mask[x]);  // (the same words for the whole wave)
        const int64_t j = (int64_t)item.begin + l, d = d0 + rank;
        if (d < 0 || d >= B) continue;  // (a malformed work list)
        for (int t = t0; t < T1; ++t) to[(int64_t)t * B + d] = from[(int64_t)t * B + j];
        out.acts[d] = src.acts[k][j];
        out.final_reward[d] = src.final_reward[k][j];
        out.lane_ids[d] = src.lane_ids[k][j];
    }
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

extern "C" int rnad_draw_columns(uint64_t seed, int source, int64_t B, int64_t b, int32_t *out) {
    RNAD_REQUIRE(out || b == 0, "rnad_draw_columns: null argument");
    RNAD_REQUIRE(B >= 1 && B <= RNAD_DRAW_MAX_LANES, "rnad_draw_columns: B = %lld outside 1 .. 2^30", (long long)B);
    RNAD_REQUIRE(b >= 0 && b <= B, "rnad_draw_columns: b = %lld outside 0 .. B = %lld", (long long)b, (long long)B);
    RNAD_REQUIRE(source >= 0, "rnad_draw_columns: negative source");
    int64_t n = 0;
    for (int64_t j = 0; j < B && n < b; ++j)
        if (rnad_draw_selected(seed, (uint32_t)source, B, b, j)) out[n++] = (int32_t)j;
    if (n != b) {  // (sigma is a bijection: cannot happen)
        set_error("rnad_draw_columns: %lld columns drawn instead of %lld", (long long)n, (long long)b);
        return 1;
    }
    return 0;
}

extern "C" int64_t rnad_bucket_draw_workspace(const rnad_tree_t *tree, int64_t B) {
    DrawPlanView p;
    if (!tree || bucket_draw_plan(tree, B, "rnad_bucket_draw_workspace", p)) return -1;
    return carve_draw(nullptr, p.max_items, (p.chunk + 63) / 64).bytes + 16;
}

extern "C" int rnad_bucket_draw_lanes(const rnad_tree_t *tree, int T_cap, int64_t B, int n, int source0, const void *const *states,
                                      const uint64_t *const *acts, const float *const *final_reward, const int32_t *const *lane_ids,
                                      const int32_t *const *items, const int32_t *const *n_items, const int64_t *b, uint64_t seed, int64_t offset,
                                      void *states_out, uint64_t *acts_out, float *final_reward_out, int32_t *lane_ids_out,
                                      int32_t *const *items_out, int32_t *const *n_items_out, double *norm, void *workspace, void *stream) {
    const char *who = "rnad_bucket_draw_lanes";
    RNAD_REQUIRE(n >= 1 && n <= RNAD_DRAW_MAX, "%s: n = %d sources outside 1 .. %d", who, n, RNAD_DRAW_MAX);
    RNAD_REQUIRE(tree && states && acts && final_reward && lane_ids && items && n_items && b && states_out && acts_out && final_reward_out &&
                     lane_ids_out && items_out && n_items_out && norm && workspace,
                 "%s: null argument", who);
    RNAD_REQUIRE(T_cap >= 1 && T_cap <= 21 && B >= 1 && source0 >= 0, "%s: bad shape (T_cap %d outside 1 .. 21, B %lld, source0 %d)", who, T_cap,
                 (long long)B, source0);
    RNAD_REQUIRE(offset >= 0 && offset <= B, "%s: offset %lld outside 0 .. B = %lld", who, (long long)offset, (long long)B);
    int64_t sum = 0;
    int sole = 0;
    for (int k = 0; k < n; ++k) {
        RNAD_REQUIRE(states[k] && acts[k] && final_reward[k] && lane_ids[k] && items[k] && n_items[k] && items_out[k] && n_items_out[k],
                     "%s: null buffer of source %d", who, k);
        RNAD_REQUIRE(b[k] >= 0 && b[k] <= B, "%s: b[%d] = %lld outside 0 .. B = %lld", who, k, (long long)b[k], (long long)B);
        sum += b[k];
        sole |= b[k] == B;  // the only source that contributes lanes: its buckets' only items may flush with plain stores
    }
    RNAD_REQUIRE(sum + offset <= B, "%s: sum b + offset = %lld exceeds B = %lld", who, (long long)(sum + offset), (long long)B);
    DrawPlanView p;
    if (int rc = bucket_draw_plan(tree, B, who, p)) return rc;
    const int words = (p.chunk + 63) / 64;
    const size_t rel = (size_t)p.rel_bytes, nB = (size_t)B, item_bytes = (size_t)p.max_items * sizeof(DrawItem);
    const DrawWork w = carve_draw((void *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15), p.max_items, words);
    struct Region {
        const void *at;
        size_t bytes;
        const char *name;
    };
    std::vector<Region> dst = {{states_out, (size_t)(T_cap + 1) * nB * rel, "states_out"}, {acts_out, nB * 8, "acts_out"},
                               {final_reward_out, nB * 4, "final_reward_out"}, {lane_ids_out, nB * 4, "lane_ids_out"},
                               {norm, 16, "norm"}, {workspace, (size_t)w.bytes + 16, "workspace"}};
    for (int k = 0; k < n; ++k) {
        dst.push_back({items_out[k], item_bytes, "items_out"});
        dst.push_back({n_items_out[k], 4, "n_items_out"});
    }
    for (int k = 0; k < n; ++k) {
        const Region from[] = {{states[k], (size_t)(T_cap + 1) * nB * rel, "states"}, {acts[k], nB * 8, "acts"},
                               {final_reward[k], nB * 4, "final_reward"}, {lane_ids[k], nB * 4, "lane_ids"},
                               {items[k], item_bytes, "items"}, {n_items[k], 4, "n_items"}};
        for (const Region &d : dst)
            for (const Region &s : from)
                RNAD_REQUIRE(!overlap(d.at, d.bytes, s.at, s.bytes), "%s: destination %s overlaps %s of source %d", who, d.name, s.name, k);
    }
    for (size_t x = 0; x < dst.size(); ++x)
        for (size_t y = x + 1; y < dst.size(); ++y)
            RNAD_REQUIRE(!overlap(dst[x].at, dst[x].bytes, dst[y].at, dst[y].bytes), "%s: destinations %s and %s overlap", who, dst[x].name, dst[y].name);
    RNAD_REQUIRE(((uintptr_t)acts_out & 7) == 0 && ((uintptr_t)norm & 7) == 0, "%s: acts_out and norm must be 8-byte aligned", who);
    DrawSources src{};
    int64_t off = offset;
    for (int k = 0; k < RNAD_DRAW_MAX; ++k) {
        const int s = k < n ? k : 0;  // (unused entries repeat source 0: never dereferenced)
        src.states[k] = states[s];
        src.acts[k] = acts[s];
        src.final_reward[k] = final_reward[s];
        src.lane_ids[k] = lane_ids[s];
        src.items[k] = (const DrawItem *)items[s];
        src.n_items[k] = n_items[s];
        src.items_out[k] = (DrawItem *)items_out[s];
        src.n_items_out[k] = n_items_out[s];
        src.b[k] = k < n ? (int32_t)b[k] : 0;
        src.off[k] = (int32_t)off;
        if (k < n) off += b[k];
    }
    const DrawOut out{states_out, acts_out, final_reward_out, lane_ids_out, norm};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)p.max_items, (unsigned)n);
    const size_t scan_lds = 2 * ((size_t)p.n_buckets + 1) * sizeof(int32_t);
    if (scan_lds > 48 * 1024)
        RNAD_HIP_OK(hipFuncSetAttribute((const void *)k_draw_scan, hipFuncAttributeMaxDynamicSharedMemorySize, (int)scan_lds));
    if (p.rel_bytes == 1) {
        hipLaunchKernelGGL((k_draw_count<uint8_t>), grid, dim3(kThreads), 0, s, src, T_cap, B, seed, source0, p.n_groups, p.n_buckets, p.shared_root,
                           p.bucket_path, words, p.max_items, w);
    } else {
        hipLaunchKernelGGL((k_draw_count<uint16_t>), grid, dim3(kThreads), 0, s, src, T_cap, B, seed, source0, p.n_groups, p.n_buckets, p.shared_root,
                           p.bucket_path, words, p.max_items, w);
    }
    hipLaunchKernelGGL(k_draw_scan, dim3((unsigned)n), dim3(kScanThreads), scan_lds, s, src, p.n_buckets, p.chunk, p.max_items, sole, w);
    if (p.rel_bytes == 1) {
        hipLaunchKernelGGL((k_draw_gather<uint8_t>), grid, dim3(kThreads), 0, s, src, n, T_cap + 1, B, offset, p.n_groups, p.n_buckets, p.shared_root,
                           p.bucket_path, words, p.max_items, w, out);
    } else {
        hipLaunchKernelGGL((k_draw_gather<uint16_t>), grid, dim3(kThreads), 0, s, src, n, T_cap + 1, B, offset, p.n_groups, p.n_buckets, p.shared_root,
                           p.bucket_path, words, p.max_items, w, out);
    }
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}
