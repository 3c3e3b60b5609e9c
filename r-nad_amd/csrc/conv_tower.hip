// conv_tower.hip -- the ConvNet of nn/net.py:88-269 (CrossConv pre-layer, residual CrossConv tower, policy and value heads) as
// fp32-MFMA kernels over a row list (gfx950).  batch_norm=False nets only; citations are baskuit/R-NaD file:line.
//
// A CrossConv (net.py:122-143) is a (1, 2A-1) and a (2A-1, 1) convolution over a zero-padded A x A board, summed.  Only in-range taps
// contribute, so each is a dense product with a Toeplitz-expanded weight:
//     row:  out[o,i,j] += sum_{c,j'} Trow[(o,j),(c,j')] in[c,i,j']     Trow[(o,j),(c,j')] = Wr[o,c,j'-j+A-1]     one product per board row i
//     col:  out[o,i,j] += sum_{c,i'} Tcol[(o,i),(c,i')] in[c,i',j]     Tcol[(o,i),(c,i')] = Wc[o,c,i'-i+A-1]     one product per board column j
// i.e. A taps per output where the padded convolution does 2A-1.  With M = Ch*A outputs and K = Cin*A inputs per product
// (48 x 48 at A = 3, Ch = 16) they tile v_mfma_f32_16x16x4_f32: M in tiles of 16, K in steps of 4, and the N = 16 columns of a tile
// are 16 SAMPLES (the activations of a sample tile live in LDS as act[sample][(c,i,j)], sample stride odd).
//
// Operand order (guide: A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C: col = l & 15, row = 4 (l >> 4) + reg):
//   A operand  lane l of (m-tile mt, k-step ks): T[16 mt + (l & 15)][4 ks + (l >> 4)] -- the packed image stores exactly these 64 floats
//              per (mt, ks), so a wave reads its operand with one coalesced 256-byte load (global memory: the image is shared by all
//              workgroups and stays in L2; it is streamed per layer, never staged whole, so its size is not bounded by the LDS)
//   B operand  lane l: act[sample l & 15][(c, b, x)]  with (c, x) = divmod(4 ks + (l >> 4), A) and b the board row / column of the product
//   C          lane l holds sample l & 15 and outputs m = 16 mt + 4 (l >> 4) + r
// The row <-> column view change between the two products goes through LDS: the row product stores (acc + bias) into a scratch
// activation buffer, the column product adds its accumulators to it in its epilogue (every element is owned by one lane) and applies
// relu / the residual there.
//
// Backward recomputes the activations of a 16-sample tile into LDS, then walks the tower back: the data gradient of a CrossConv is a
// CrossConv with the transposed Toeplitz operands (a second set of images in the packed buffer), the weight gradient is the product
// gT[(o,y),(c,x)] = sum_{sample,b} dz[sample,(o,b,y)] in[sample,(c,b,x)] contracted over K = 16 A on the matrix cores.  Every workgroup
// accumulates its Toeplitz-shaped partials in a private slice of the caller's workspace (fixed owner lane per element, tiles in a fixed
// order); one reduction kernel folds the Toeplitz diagonals and sums the workgroups in ascending order -- no float atomics, bitwise
// reproducible.
#include "common.hpp"
#include "conv_shape.hpp"
#include "rollout_math.hpp"

#include <algorithm>
#include <type_traits>

using namespace rnad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kConvThreads = 256, kConvWaves = kConvThreads / 64;
constexpr int kConvBwdGrid = 256;   // workgroups of the backward launch = partial slices of the reduction
constexpr int kConvFwdGrid = 1024;
constexpr size_t kConvLds = 160 * 1024;

// fp16 observation tables (ObsT = __half): the observations of the NS samples from `first` on, converted to the fp32 the tower computes
// with, -> dst[s * stride + f]; zeros past sample N.  The table holds rounded values and v_cvt_f32_f16 is exact, subnormals included, so
// the kernels on a half table give the bits of the float kernels on the up-converted table.  Read as __half2 pairs: a row is 4 A^2 bytes,
// so in a 4-byte aligned table (the entry points check) every row starts on a pair.
__device__ __forceinline__ void stage_half_obs(float *dst, int stride, int NS, int A, int64_t first, int64_t N, const int32_t *__restrict__ rows,
                                               const __half *__restrict__ obs) {
    const __half2 *__restrict__ obs2 = reinterpret_cast<const __half2 *>(obs);
    const int O2 = A * A;
    for (int idx = threadIdx.x; idx < NS * O2; idx += kConvThreads) {
        const int s = idx / O2, f = idx % O2;
        const int64_t sample = first + s;
        float2 x = float2{0.0f, 0.0f};
        if (sample < N) x = __half22float2(obs2[(rows ? (int64_t)rows[sample] : sample) * O2 + f]);
        dst[s * stride + 2 * f] = x.x;
        dst[s * stride + 2 * f + 1] = x.y;
    }
}

__device__ __forceinline__ int board_index(int A, int dir, int ch, int b, int x) { return dir == 0 ? (ch * A + b) * A + x : (ch * A + x) * A + b; }

// One direction of a CrossConv over NT 16-sample tiles: every (board line b, m-tile) is a job of one wave; epi(sample, f, channel,
// value) receives the product for output element f = (channel, i, j) of the sample.
template <int NT, typename Epi>
__device__ __forceinline__ void conv_dir(const ConvShape &sh, const float *__restrict__ img, int KSl, int Kreal, int dir, const float *in, int inP,
                                         Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = sh.A, n = lane & 15, kq = lane >> 4;
    for (int job = wave; job < A * sh.Mt; job += kConvWaves) {
        const int b = job / sh.Mt, mt = job % sh.Mt;
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *__restrict__ ap = img + (size_t)mt * KSl * 64 + lane;
        for (int ks = 0; ks < KSl; ++ks) {
            const float a = ap[ks * 64];
            const int k = 4 * ks + kq;
            const bool ok = k < Kreal;
            const int f = ok ? board_index(A, dir, k / A, b, k % A) : 0;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float x = in[(nt * 16 + n) * inP + f];
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok ? x : 0.0f, acc[nt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mt * 16 + kq * 4 + r;
            const int o = m / A, f = board_index(A, dir, o, b, m % A);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) epi(nt * 16 + n, f, o, acc[nt][r]);
        }
    }
}

// A whole CrossConv: tmp = row product + bias; epi(sample, f, tmp + column product).  `tmp` may be the buffer epi writes.
template <int NT, typename Epi>
__device__ __forceinline__ void cross_conv(const ConvShape &sh, const float *__restrict__ img, const float *__restrict__ bias, int KSl, int Kreal,
                                           const float *in, int inP, float *tmp, Epi epi) {
    const int P = sh.P;
    conv_dir<NT>(sh, img, KSl, Kreal, 0, in, inP, [&](int s, int f, int o, float v) { tmp[s * P + f] = bias ? v + bias[o] : v; });
    __syncthreads();
    conv_dir<NT>(sh, img + sh.Mt * KSl * 64, KSl, Kreal, 1, in, inP, [&](int s, int f, int, float v) { epi(s, f, tmp[s * P + f] + v); });
    __syncthreads();
}

// Epilogues of k_conv_forward, after the heads of a sample tile.  FwdPlain: nothing more.  FwdActor<A> (rnad_conv_forward_actor): the net
// is a tabular ACTOR -- the heads also park the A logits of a sample in U (free once the tower is done; sample stride P, odd: the
// 32 samples of a half-wave sit on 32 banks for the stores here and the loads below), and one thread per sample turns them into the
// sample's padded policy row under the mover's legal bits (net.py:225-227 as policy_head): the same function of the same logits as
// k_policy_rows / k_row_records and the epilogue of k_mlp_forward.
struct FwdPlain {
    static constexpr int kA = 0;
};
template <int A>
struct FwdActor {
    static constexpr int kA = A;
    float *__restrict__ policy_rows;        // [2S, (A + 3) & ~3], 16-byte aligned
    const uint8_t *__restrict__ mask_tab;   // [2S]
};

template <int NT, typename Epi, typename ObsT>
__global__ __launch_bounds__(kConvThreads) void k_conv_forward(int64_t N, const int32_t *__restrict__ rows, const int64_t *__restrict__ n_rows,
                                                               ConvShape sh, const float *__restrict__ packed, const ObsT *__restrict__ obs,
                                                               float *__restrict__ logits, float *__restrict__ value, Epi epi) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (n_rows) N = *n_rows < N ? *n_rows : N;  // the list never exceeds its capacity
    constexpr int NS = NT * 16;
    const int A = sh.A, P = sh.P, F = sh.F, OBS = 2 * A * A, KA = sh.Ch * A;
    float *H = lds, *T = H + NS * P, *U = T + NS * P;
    const int64_t n_tiles = (N + NS - 1) / NS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        if constexpr (std::is_same<ObsT, __half>::value) {
            stage_half_obs(T, P, NS, A, tile * NS, N, rows, obs);
        } else {
            for (int idx = threadIdx.x; idx < NS * OBS; idx += kConvThreads) {
                const int s = idx / OBS, f = idx % OBS;
                const int64_t sample = tile * NS + s;
                float x = 0.0f;
                if (sample < N) x = obs[(rows ? (int64_t)rows[sample] : sample) * OBS + f];
                T[s * P + f] = x;
            }
        }
        __syncthreads();
        cross_conv<NT>(sh, packed + sh.fwd(0), packed + sh.bias(0), sh.KS0, 2 * A, T, P, U, [&](int s, int f, float v) { H[s * P + f] = v; });
        for (int d = 0; d < sh.D; ++d) {
            const int l0 = 1 + 2 * d, l1 = 2 + 2 * d;
            cross_conv<NT>(sh, packed + sh.fwd(l0), packed + sh.bias(l0), sh.KS, KA, H, P, T, [&](int s, int f, float v) { T[s * P + f] = fmaxf(v, 0.0f); });
            cross_conv<NT>(sh, packed + sh.fwd(l1), packed + sh.bias(l1), sh.KS, KA, T, P, U, [&](int s, int f, float v) { H[s * P + f] += fmaxf(v, 0.0f); });
        }
        // heads (net.py:220-225): one thread per (sample, output), flatten order (c, i, j)
        for (int idx = threadIdx.x; idx < NS * (A + 1); idx += kConvThreads) {
            const int s = idx % NS, a = idx / NS;
            const int64_t sample = tile * NS + s;
            if (sample >= N) continue;
            const bool is_value = a == A;
            float *out = is_value ? value : logits;
            if (!out) continue;
            const float *__restrict__ w = packed + (is_value ? sh.wv() : sh.wp() + a * F);
            const float *h = H + s * P;
            float acc = 0.0f;
            for (int f = 0; f < F; ++f) acc += w[f] * h[f];
            acc += packed[is_value ? sh.bv() : sh.bp() + a];
            const int64_t row = rows ? (int64_t)rows[sample] : sample;
            if (is_value) out[row] = acc;
            else out[row * A + a] = acc;
            if constexpr (Epi::kA > 0) {
                if (!is_value) U[s * P + a] = acc;
            }
        }
        if constexpr (Epi::kA > 0) {
            constexpr int kA = Epi::kA, PS = (kA + 3) & ~3;
            __syncthreads();
            for (int s = threadIdx.x; s < NS; s += kConvThreads) {
                const int64_t sample = tile * NS + s;
                if (sample >= N) continue;
                const int64_t row = rows ? (int64_t)rows[sample] : sample;
                float lg[kA], pol[PS];
#pragma unroll
                for (int a = 0; a < kA; ++a) lg[a] = U[s * P + a];
                rnad::dev::policy_head_ptr<kA>(lg, epi.mask_tab[row], pol, nullptr);
#pragma unroll
                for (int a = kA; a < PS; ++a) pol[a] = 0.0f;
                float4 *p4 = reinterpret_cast<float4 *>(epi.policy_rows + row * PS);
#pragma unroll
                for (int u = 0; u < PS / 4; ++u) p4[u] = float4{pol[4 * u], pol[4 * u + 1], pol[4 * u + 2], pol[4 * u + 3]};
            }
        }
        __syncthreads();
    }
}

// gT[(o,y),(c,x)] += sum_{sample, b} dz[sample,(o,b,y)] in[sample,(c,b,x)] for both directions of layer l, into this workgroup's slice.
__device__ __forceinline__ void weight_grad(const ConvShape &sh, float *__restrict__ part, int ncols, const float *dz, const float *in, int inP) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int A = sh.A, P = sh.P, q = lane & 15, kq = lane >> 4;
    const int Nt = (ncols + 15) / 16;
    for (int job = wave; job < 2 * sh.Mt * Nt; job += kConvWaves) {
        const int dir = job / (sh.Mt * Nt), mt = (job / Nt) % sh.Mt, nt = job % Nt;
        const int m = mt * 16 + q, nn = nt * 16 + q;
        const bool okn = nn < ncols;
        const int o = m / A, y = m % A, c = okn ? nn / A : 0, x = okn ? nn % A : 0;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < 4 * A; ++ks) {
            const int k = 4 * ks + kq, b = k >> 4, s = k & 15;
            const float a = dz[s * P + board_index(A, dir, o, b, y)];
            const float v = in[s * inP + board_index(A, dir, c, b, x)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, okn ? v : 0.0f, acc, 0, 0, 0);
        }
        if (okn) {
            float *__restrict__ dst = part + dir * sh.M * ncols + nn;
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(mt * 16 + kq * 4 + r) * ncols] += acc[r];
        }
    }
}

// gb[o] += sum_{sample,i,j} dz[sample,o,i,j]: 16 lanes per channel (one per sample), summed in a fixed shuffle tree.
__device__ __forceinline__ void bias_grad(const ConvShape &sh, float *__restrict__ part_bias, const float *dz) {
    const int AA = sh.A * sh.A;
    for (int idx = threadIdx.x; idx < sh.Ch * 16; idx += kConvThreads) {
        const int o = idx >> 4, s = idx & 15;
        const float *z = dz + s * sh.P + o * AA;
        float sum = 0.0f;
        for (int e = 0; e < AA; ++e) sum += z[e];
        sum += __shfl_xor(sum, 8, 64);
        sum += __shfl_xor(sum, 4, 64);
        sum += __shfl_xor(sum, 2, 64);
        sum += __shfl_xor(sum, 1, 64);
        if (s == 0) part_bias[o] += sum;
    }
}

template <bool LEAN, typename ObsT>
__global__ __launch_bounds__(kConvThreads) void k_conv_backward(int64_t N, const int32_t *__restrict__ rows, const int64_t *__restrict__ n_rows,
                                                                ConvShape sh, const float *__restrict__ packed, const ObsT *__restrict__ obs,
                                                                const float *__restrict__ dlogits, const float *__restrict__ dvalue,
                                                                float *__restrict__ workspace) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (n_rows) N = *n_rows < N ? *n_rows : N;
    constexpr int NS = 16;
    const int A = sh.A, P = sh.P, XP = sh.XP, F = sh.F, D = sh.D, OBS = 2 * A * A, KA = sh.Ch * A, A1 = A + 1;
    // saved activations: H[0..D] (the residual stream), T[d] = relu(conv0), R[d] = relu(conv1) -- the last block's R is written
    // straight into Gz, where the walk back turns it into dz1 in place; gradient buffers G, Gz, U
    // LEAN: H[0..D-1] and ONE T buffer; H_D is written into Gz (dead once the heads are done), T[d] and R[d] are recomputed per block
    float *Hs = lds, *Ts = Hs + (LEAN ? D : D + 1) * NS * P, *Rs = Ts + (LEAN ? 1 : D) * NS * P;
    float *G = LEAN ? Rs : Rs + (D - 1) * NS * P, *Gz = G + NS * P, *U = Gz + NS * P, *X = U + NS * P, *DL = X + NS * XP;
    float *__restrict__ part = workspace + (size_t)blockIdx.x * sh.part_total();
    for (int i = threadIdx.x; i < sh.part_total(); i += kConvThreads) part[i] = 0.0f;
    __syncthreads();
    const int64_t n_tiles = (N + NS - 1) / NS;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // inputs of the tile; samples past the end carry zero gradients and so contribute nothing
        if constexpr (std::is_same<ObsT, __half>::value) {
            stage_half_obs(X, XP, NS, A, tile * NS, N, rows, obs);
        } else {
            for (int idx = threadIdx.x; idx < NS * OBS; idx += kConvThreads) {
                const int s = idx / OBS, f = idx % OBS;
                const int64_t sample = tile * NS + s;
                X[s * XP + f] = sample < N ? obs[(rows ? (int64_t)rows[sample] : sample) * OBS + f] : 0.0f;
            }
        }
        for (int idx = threadIdx.x; idx < NS * A1; idx += kConvThreads) {
            const int s = idx / A1, a = idx % A1;
            const int64_t sample = tile * NS + s;
            float g = 0.0f;
            if (sample < N) {
                const int64_t row = rows ? (int64_t)rows[sample] : sample;
                g = a < A ? dlogits[row * A + a] : dvalue[row];
            }
            DL[s * A1 + a] = g;
        }
        __syncthreads();
        // ---- forward, activations kept
        cross_conv<1>(sh, packed + sh.fwd(0), packed + sh.bias(0), sh.KS0, 2 * A, X, XP, U, [&](int s, int f, float v) { Hs[s * P + f] = v; });
        for (int d = 0; d < D; ++d) {
            const int l0 = 1 + 2 * d, l1 = 2 + 2 * d;
            if constexpr (LEAN) {
                float *H = Hs + d * NS * P, *Hn = d == D - 1 ? Gz : H + NS * P, *T = Ts;
                cross_conv<1>(sh, packed + sh.fwd(l0), packed + sh.bias(l0), sh.KS, KA, H, P, T, [&](int s, int f, float v) { T[s * P + f] = fmaxf(v, 0.0f); });
                cross_conv<1>(sh, packed + sh.fwd(l1), packed + sh.bias(l1), sh.KS, KA, T, P, U,
                              [&](int s, int f, float v) { Hn[s * P + f] = H[s * P + f] + fmaxf(v, 0.0f); });
                continue;
            }
            float *H = Hs + d * NS * P, *Hn = H + NS * P, *T = Ts + d * NS * P, *R = d == D - 1 ? Gz : Rs + d * NS * P;
            cross_conv<1>(sh, packed + sh.fwd(l0), packed + sh.bias(l0), sh.KS, KA, H, P, T, [&](int s, int f, float v) { T[s * P + f] = fmaxf(v, 0.0f); });
            cross_conv<1>(sh, packed + sh.fwd(l1), packed + sh.bias(l1), sh.KS, KA, T, P, U, [&](int s, int f, float v) {
                const float r = fmaxf(v, 0.0f);
                R[s * P + f] = r;
                Hn[s * P + f] = H[s * P + f] + r;
            });
        }
        // ---- heads: G = dL/dh_D, partials of the head weights
        {
            const float *HD = LEAN ? Gz : Hs + D * NS * P;
            for (int idx = threadIdx.x; idx < NS * F; idx += kConvThreads) {
                const int s = idx / F, f = idx % F;
                float g = packed[sh.wv() + f] * DL[s * A1 + A];
                for (int a = 0; a < A; ++a) g += packed[sh.wp() + a * F + f] * DL[s * A1 + a];
                G[s * P + f] = g;
            }
            for (int idx = threadIdx.x; idx < A1 * F; idx += kConvThreads) {
                const int a = idx / F, f = idx % F;
                float g = 0.0f;
                for (int s = 0; s < NS; ++s) g += DL[s * A1 + a] * HD[s * P + f];
                part[(a < A ? sh.part_wp() + a * F : sh.part_wv()) + f] += g;
            }
            if (threadIdx.x < A1) {
                const int a = threadIdx.x;
                float g = 0.0f;
                for (int s = 0; s < NS; ++s) g += DL[s * A1 + a];
                part[a < A ? sh.part_bp() + a : sh.part_bv()] += g;
            }
        }
        __syncthreads();
        // ---- the tower, last block first
        for (int d = D - 1; d >= 0; --d) {
            const int l0 = 1 + 2 * d, l1 = 2 + 2 * d;
            const float *H = Hs + d * NS * P, *T = LEAN ? Ts : Ts + d * NS * P, *R = (LEAN || d == D - 1) ? Gz : Rs + d * NS * P;
            if constexpr (LEAN) {  // relu(conv0) and relu(conv1) of this block once more: the same products, the same bits
                cross_conv<1>(sh, packed + sh.fwd(l0), packed + sh.bias(l0), sh.KS, KA, H, P, Ts, [&](int s, int f, float v) { Ts[s * P + f] = fmaxf(v, 0.0f); });
                cross_conv<1>(sh, packed + sh.fwd(l1), packed + sh.bias(l1), sh.KS, KA, Ts, P, U, [&](int s, int f, float v) { Gz[s * P + f] = fmaxf(v, 0.0f); });
            }
            for (int idx = threadIdx.x; idx < NS * F; idx += kConvThreads) {
                const int e = (idx / F) * P + idx % F;
                Gz[e] = R[e] > 0.0f ? G[e] : 0.0f;  // dz1
            }
            __syncthreads();
            weight_grad(sh, part + sh.part(l1), KA, Gz, T, P);
            bias_grad(sh, part + sh.part_bias(l1), Gz);
            cross_conv<1>(sh, packed + sh.tr(l1), nullptr, sh.KS, KA, Gz, P, U, [&](int s, int f, float v) { U[s * P + f] = T[s * P + f] > 0.0f ? v : 0.0f; });  // dz0
            weight_grad(sh, part + sh.part(l0), KA, U, H, P);
            bias_grad(sh, part + sh.part_bias(l0), U);
            cross_conv<1>(sh, packed + sh.tr(l0), nullptr, sh.KS, KA, U, P, Gz, [&](int s, int f, float v) { G[s * P + f] += v; });
        }
        weight_grad(sh, part + sh.part(0), 2 * A, G, X, XP);
        bias_grad(sh, part + sh.part_bias(0), G);
        __syncthreads();
    }
}

// Fold the Toeplitz diagonals and sum the workgroups' slices in ascending order: one thread per parameter of the flat bucket.
__global__ __launch_bounds__(kConvThreads) void k_conv_reduce(ConvShape sh, int n_parts, const float *__restrict__ workspace, float *__restrict__ grads) {
    int e = blockIdx.x * kConvThreads + threadIdx.x;
    if (e >= sh.n_params()) return;
    const int out = e, A = sh.A, T = 2 * A - 1;
    const size_t stride = sh.part_total();
    int base = 0, step = 0, first = 0, count = 1;  // the element sums `count` partial entries base + first * step ... per slice
    bool found = false;
    for (int l = 0; l < sh.L && !found; ++l) {
        const int cin = sh.cin(l), ncols = sh.ncols(l), ws = sh.wsize(l);
        for (int dir = 0; dir < 2 && !found; ++dir) {
            found = e < ws + sh.Ch;
            if (e < ws) {
                const int o = e / (cin * T), c = (e / T) % cin, k = e % T;
                // entries (o, y), (c, x) with x - y + A - 1 = k
                const int y0 = max(0, A - 1 - k), y1 = min(A - 1, 2 * A - 2 - k);
                base = sh.part(l) + dir * sh.M * ncols + (o * A) * ncols + c * A + (k - (A - 1));
                step = ncols + 1; first = y0; count = y1 - y0 + 1;
            } else if (e < ws + sh.Ch) {
                base = sh.part_bias(l) + (e - ws);
            }
            e -= ws + sh.Ch;
        }
    }
    if (!found) {  // policy.weight, policy.bias, value.weight, value.bias
        const int F = sh.F;
        if (e < A * F) base = sh.part_wp() + e;
        else if (e < A * F + A) base = sh.part_bp() + (e - A * F);
        else if (e < A * F + A + F) base = sh.part_wv() + (e - A * F - A);
        else base = sh.part_bv();
    }
    float sum = 0.0f;
    for (int g = 0; g < n_parts; ++g) {
        const float *__restrict__ p = workspace + g * stride + base;
        for (int i = 0; i < count; ++i) sum += p[(first + i) * step];
    }
    grads[out] = sum;
}

struct ConvWeights {
    const float *w[kConvMaxTensors];
};

// Reference-layout tensors (net.parameters() order) -> the packed image.
__global__ __launch_bounds__(kConvThreads) void k_conv_pack(ConvShape sh, ConvWeights ws, float *__restrict__ packed) {
    const int i = blockIdx.x * kConvThreads + threadIdx.x;
    if (i >= sh.packed_total()) return;
    const int A = sh.A, T = 2 * A - 1, L = sh.L;
    float x = 0.0f;
    if (i < sh.fwd(L)) {
        int l = 0;
        while (i >= sh.fwd(l + 1)) ++l;
        const int r = i - sh.fwd(l), img = sh.image(l), KSl = sh.ks(l), cin = sh.cin(l);
        if (r < 2 * img) {
            const int dir = r / img, q = r % img;
            const int mt = q / (KSl * 64), ks = (q / 64) % KSl, lane = q % 64;
            const int m = mt * 16 + (lane & 15), k = 4 * ks + (lane >> 4);
            if (k < cin * A) x = ws.w[4 * l + 2 * dir][((m / A) * cin + k / A) * T + (k % A) - (m % A) + A - 1];
        } else {
            x = ws.w[4 * l + 1][r - 2 * img] + ws.w[4 * l + 3][r - 2 * img];
        }
    } else if (i < sh.wp()) {  // transposed operands of the tower layers: T'[(c,x),(o,y)] = W[o,c,x-y+A-1]
        const int img = sh.image(1), r = i - sh.fwd(L);
        const int l = 1 + r / (2 * img), dir = (r / img) % 2, q = r % img;
        const int mt = q / (sh.KS * 64), ks = (q / 64) % sh.KS, lane = q % 64;
        const int m = mt * 16 + (lane & 15), k = 4 * ks + (lane >> 4);
        x = ws.w[4 * l + 2 * dir][((k / A) * sh.Ch + m / A) * T + (m % A) - (k % A) + A - 1];
    } else if (i < sh.wv()) {
        x = ws.w[4 * L][i - sh.wp()];
    } else if (i < sh.bp()) {
        x = ws.w[4 * L + 2][i - sh.wv()];
    } else if (i < sh.bv()) {
        x = ws.w[4 * L + 1][i - sh.bp()];
    } else if (i == sh.bv()) {
        x = ws.w[4 * L + 3][0];
    }
    packed[i] = x;
}

int fwd_tiles(const ConvShape &sh) {
    for (int nt = 4; nt >= 1; nt >>= 1)
        if (sh.fwd_lds(nt) <= kConvLds) return nt;
    return 0;
}

bool conv_shape_ok(int A, int Ch, int depth) {
    if (A < 1 || A > RNAD_MAX_ACTIONS || Ch < 2 || Ch > 256 || depth < 1 || depth > kConvMaxDepth || (Ch * A) % 16 != 0) return false;
    const ConvShape sh(A, Ch, depth);
    return fwd_tiles(sh) > 0 && (sh.bwd_lds() <= kConvLds || sh.bwd_lds_lean() <= kConvLds);
}

}  // namespace

extern "C" int rnad_conv_supported(int A, int Ch, int depth) { return conv_shape_ok(A, Ch, depth) ? 1 : 0; }

extern "C" int64_t rnad_conv_packed_size(int A, int Ch, int depth) { return conv_shape_ok(A, Ch, depth) ? ConvShape(A, Ch, depth).packed_total() : -1; }

extern "C" int64_t rnad_conv_param_count(int A, int Ch, int depth) { return conv_shape_ok(A, Ch, depth) ? ConvShape(A, Ch, depth).n_params() : -1; }

extern "C" int rnad_conv_pack(int A, int Ch, int depth, const float *const *weights, float *packed, void *stream) {
    RNAD_REQUIRE(conv_shape_ok(A, Ch, depth), "rnad_conv_pack: unsupported shape (A=%d, channels=%d, depth=%d)", A, Ch, depth);
    RNAD_REQUIRE(weights && packed, "rnad_conv_pack: null argument");
    const ConvShape sh(A, Ch, depth);
    ConvWeights ws{};
    for (int j = 0; j < 4 * sh.L + 4; ++j) {
        RNAD_REQUIRE(weights[j], "rnad_conv_pack: null weight tensor %d", j);
        ws.w[j] = weights[j];
    }
    hipLaunchKernelGGL(k_conv_pack, dim3((sh.packed_total() + kConvThreads - 1) / kConvThreads), dim3(kConvThreads), 0, (hipStream_t)stream, sh, ws,
                       packed);
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}

// One launch of k_conv_forward<NT, Epi, ObsT> over N rows (or the row list), NT from fwd_tiles.
template <typename Epi, typename ObsT>
static int conv_forward_launch(int64_t N, const int32_t *rows, const int64_t *n_rows, const ConvShape &sh, const float *packed, const ObsT *obs,
                               float *logits, float *value, Epi epi, void *stream) {
    if (N == 0) return 0;
    const int nt = fwd_tiles(sh);
    const size_t lds = sh.fwd_lds(nt);
    const int64_t n_tiles = (N + nt * 16 - 1) / (nt * 16);
    const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, kConvFwdGrid);
#define RNAD_CONV_FWD(NT_)                                                                                                                  \
    do {                                                                                                                                    \
        auto kern = k_conv_forward<NT_, Epi, ObsT>;                                                                                         \
        if (lds > 64 * 1024) RNAD_HIP_OK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));    \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kConvThreads), lds, (hipStream_t)stream, N, rows, n_rows, sh, packed, obs, logits, value, \
                           epi);                                                                                                            \
    } while (0)
    if (nt == 4) RNAD_CONV_FWD(4);
    else if (nt == 2) RNAD_CONV_FWD(2);
    else RNAD_CONV_FWD(1);
#undef RNAD_CONV_FWD
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}

// obs_half: the observations are fp16 (rounded values, converted as a tile is staged: the arithmetic stays fp32), as in the MLP entry points.
extern "C" int rnad_conv_forward_obs(int64_t N, const int32_t *rows, const int64_t *n_rows, int A, int Ch, int depth, const float *packed,
                                     const void *obs, int obs_half, float *logits, float *value, void *stream) {
    RNAD_REQUIRE(conv_shape_ok(A, Ch, depth), "rnad_conv_forward: unsupported shape (A=%d, channels=%d, depth=%d)", A, Ch, depth);
    RNAD_REQUIRE(packed && obs && (logits || value), "rnad_conv_forward: null argument");
    RNAD_REQUIRE(!rows == !n_rows, "rnad_conv_forward: rows and n_rows go together");
    RNAD_REQUIRE(N >= 0, "rnad_conv_forward: negative batch");
    RNAD_REQUIRE(!obs_half || ((uintptr_t)obs & 3) == 0, "rnad_conv_forward: an fp16 table must be 4-byte aligned");
    const ConvShape sh(A, Ch, depth);
    if (obs_half) return conv_forward_launch(N, rows, n_rows, sh, packed, (const __half *)obs, logits, value, FwdPlain{}, stream);
    return conv_forward_launch(N, rows, n_rows, sh, packed, (const float *)obs, logits, value, FwdPlain{}, stream);
}

extern "C" int rnad_conv_forward(int64_t N, const int32_t *rows, const int64_t *n_rows, int A, int Ch, int depth, const float *packed,
                                 const float *obs, float *logits, float *value, void *stream) {
    return rnad_conv_forward_obs(N, rows, n_rows, A, Ch, depth, packed, obs, 0, logits, value, stream);
}

// A tabular ACTOR on (a row list of) the tree's 2S observations: rnad_conv_forward's logits and value (the same kernel, the same bits) and,
// from its epilogue, the policy rows [2S, rnad_bucket_policy_row_stride(A)] the bucketed rollout kernels gather from.  rows / n_rows:
// NULL = all 2S rows; rows that are not listed are neither read nor written.
extern "C" int rnad_conv_forward_actor_obs(const rnad_tree_t *tree, const int32_t *rows, const int64_t *n_rows, int Ch, int depth,
                                           const float *packed, const void *obs, int obs_half, float *logits, float *value, float *policy_rows,
                                           void *stream) {
    RNAD_REQUIRE(tree && packed && obs && logits && value && policy_rows, "rnad_conv_forward_actor: null argument");
    RNAD_REQUIRE(conv_shape_ok(tree->A, Ch, depth), "rnad_conv_forward_actor: unsupported shape (A=%d, channels=%d, depth=%d)", tree->A, Ch, depth);
    RNAD_REQUIRE(!rows == !n_rows, "rnad_conv_forward_actor: rows and n_rows go together");
    RNAD_REQUIRE(((uintptr_t)policy_rows & 15) == 0, "rnad_conv_forward_actor: policy_rows must be 16-byte aligned");
    RNAD_REQUIRE(!obs_half || ((uintptr_t)obs & 3) == 0, "rnad_conv_forward_actor: an fp16 table must be 4-byte aligned");
    const ConvShape sh(tree->A, Ch, depth);
    RNAD_DISPATCH_A(tree->A, {
        FwdActor<kA> epi{policy_rows, tree->mask_tab};
        const int rc = obs_half ? conv_forward_launch(2 * tree->S, rows, n_rows, sh, packed, (const __half *)obs, logits, value, epi, stream)
                                : conv_forward_launch(2 * tree->S, rows, n_rows, sh, packed, (const float *)obs, logits, value, epi, stream);
        if (rc) return rc;
    });
    return 0;
}

extern "C" int rnad_conv_forward_actor(const rnad_tree_t *tree, const int32_t *rows, const int64_t *n_rows, int Ch, int depth, const float *packed,
                                       const float *obs, float *logits, float *value, float *policy_rows, void *stream) {
    return rnad_conv_forward_actor_obs(tree, rows, n_rows, Ch, depth, packed, obs, 0, logits, value, policy_rows, stream);
}

static int conv_bwd_grid(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 15) / 16, kConvBwdGrid)); }

extern "C" int64_t rnad_conv_backward_workspace(int64_t N, int A, int Ch, int depth) {
    if (!conv_shape_ok(A, Ch, depth) || N < 0) return -1;
    return (int64_t)conv_bwd_grid(N) * ConvShape(A, Ch, depth).part_total() * (int64_t)sizeof(float);
}

// One launch of k_conv_backward<LEAN, ObsT> into the workgroups' slices of `workspace`.
template <bool LEAN, typename ObsT>
static int conv_backward_launch(int grid, size_t lds, hipStream_t s, int64_t N, const int32_t *rows, const int64_t *n_rows, const ConvShape &sh,
                                const float *packed, const ObsT *obs, const float *dlogits, const float *dvalue, float *workspace) {
    auto kern = k_conv_backward<LEAN, ObsT>;
    if (lds > 64 * 1024) RNAD_HIP_OK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kConvThreads), lds, s, N, rows, n_rows, sh, packed, obs, dlogits, dvalue, workspace);
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int rnad_conv_backward_obs(int64_t N, const int32_t *rows, const int64_t *n_rows, int A, int Ch, int depth, const float *packed,
                                      const void *obs, int obs_half, const float *dlogits, const float *dvalue, float *grads, float *workspace,
                                      void *stream) {
    RNAD_REQUIRE(conv_shape_ok(A, Ch, depth), "rnad_conv_backward: unsupported shape (A=%d, channels=%d, depth=%d)", A, Ch, depth);
    RNAD_REQUIRE(packed && obs && dlogits && dvalue && grads && workspace, "rnad_conv_backward: null argument");
    RNAD_REQUIRE(!rows == !n_rows, "rnad_conv_backward: rows and n_rows go together");
    RNAD_REQUIRE(N >= 0, "rnad_conv_backward: negative batch");
    RNAD_REQUIRE(!obs_half || ((uintptr_t)obs & 3) == 0, "rnad_conv_backward: an fp16 table must be 4-byte aligned");
    const ConvShape sh(A, Ch, depth);
    const bool lean = sh.bwd_lds() > kConvLds;  // the saved activations do not fit: recompute them per block
    const size_t lds = lean ? sh.bwd_lds_lean() : sh.bwd_lds();
    const int grid = conv_bwd_grid(N);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (obs_half) {
        const __half *o = (const __half *)obs;
        rc = lean ? conv_backward_launch<true>(grid, lds, s, N, rows, n_rows, sh, packed, o, dlogits, dvalue, workspace)
                  : conv_backward_launch<false>(grid, lds, s, N, rows, n_rows, sh, packed, o, dlogits, dvalue, workspace);
    } else {
        const float *o = (const float *)obs;
        rc = lean ? conv_backward_launch<true>(grid, lds, s, N, rows, n_rows, sh, packed, o, dlogits, dvalue, workspace)
                  : conv_backward_launch<false>(grid, lds, s, N, rows, n_rows, sh, packed, o, dlogits, dvalue, workspace);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_conv_reduce, dim3((sh.n_params() + kConvThreads - 1) / kConvThreads), dim3(kConvThreads), 0, s, sh, grid, workspace, grads);
    RNAD_HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int rnad_conv_backward(int64_t N, const int32_t *rows, const int64_t *n_rows, int A, int Ch, int depth, const float *packed,
                                  const float *obs, const float *dlogits, const float *dvalue, float *grads, float *workspace, void *stream) {
    return rnad_conv_backward_obs(N, rows, n_rows, A, Ch, depth, packed, obs, 0, dlogits, dvalue, grads, workspace, stream);
}
