// conv_shape.hpp -- sizes and offsets of one ConvNet shape (packed image, backward partials, flat parameter bucket) and the map from a
// parameter element to its slots of the packed image.  Shared by the tower kernels (conv_tower.hip: k_conv_pack is the gather), the
// optimiser tail (optim.hip: k_conv_optimizer_step is the scatter) and the host export rnad_conv_image_slots.
#pragma once

#include "common.hpp"

namespace rnad {

constexpr int kConvMaxDepth = 8;
constexpr int kConvMaxTensors = 4 * (2 * kConvMaxDepth + 1) + 4;

// Sizes and offsets of one net shape: the packed image, a workgroup's partial slice and the flat parameter bucket.
// Layer l: 0 = pre, 1 + 2 d = tower.d.conv0, 2 + 2 d = tower.d.conv1.
struct ConvShape {
    int A, Ch, D, L;
    int F, P, XP;      // floats per sample of an activation, its LDS stride (odd), the LDS stride of an observation
    int M, Mt, KS, KS0;  // outputs per product, their tiles, k-steps of a tower product and of the pre-layer's (K = 2 A, zero padded)
    __host__ __device__ ConvShape(int A_, int Ch_, int D_) : A(A_), Ch(Ch_), D(D_), L(2 * D_ + 1) {
        F = Ch * A * A; P = F | 1; XP = (2 * A * A) | 1;
        M = Ch * A; Mt = M / 16; KS = M / 4; KS0 = (2 * A + 3) / 4;
    }
    __host__ __device__ int cin(int l) const { return l ? Ch : 2; }
    __host__ __device__ int ks(int l) const { return l ? KS : KS0; }
    __host__ __device__ int image(int l) const { return Mt * ks(l) * 64; }  // one Toeplitz operand image
    // packed: per layer [row image][column image][bias br + bc], then the transposed images of the tower layers, then the heads
    __host__ __device__ int fwd(int l) const { return l == 0 ? 0 : (2 * Mt * KS0 * 64 + Ch) + (l - 1) * (2 * Mt * KS * 64 + Ch); }
    __host__ __device__ int bias(int l) const { return fwd(l) + 2 * image(l); }
    __host__ __device__ int tr(int l) const { return fwd(L) + (l - 1) * 2 * Mt * KS * 64; }  // l >= 1
    __host__ __device__ int wp() const { return tr(L); }
    __host__ __device__ int wv() const { return wp() + A * F; }
    __host__ __device__ int bp() const { return wv() + F; }
    __host__ __device__ int bv() const { return bp() + A; }
    __host__ __device__ int packed_total() const { return (bv() + 1 + 3) & ~3; }
    // a workgroup's partials: per layer [gTrow M x Cin A][gTcol M x Cin A][bias Ch], then gWp [A, F], gWv [F], gbp [A], gbv
    __host__ __device__ int ncols(int l) const { return cin(l) * A; }
    __host__ __device__ int part(int l) const { return l == 0 ? 0 : (2 * M * 2 * A + Ch) + (l - 1) * (2 * M * M + Ch); }
    __host__ __device__ int part_bias(int l) const { return part(l) + 2 * M * ncols(l); }
    __host__ __device__ int part_wp() const { return part(L); }
    __host__ __device__ int part_wv() const { return part_wp() + A * F; }
    __host__ __device__ int part_bp() const { return part_wv() + F; }
    __host__ __device__ int part_bv() const { return part_bp() + A; }
    __host__ __device__ int part_total() const { return part_bv() + 1; }
    // the flat bucket, net.parameters() order
    __host__ __device__ int wsize(int l) const { return Ch * cin(l) * (2 * A - 1); }
    __host__ __device__ int n_params() const { return 2 * (wsize(0) + Ch) + 2 * D * 2 * (wsize(1) + Ch) + A * F + A + F + 1; }
    __host__ __device__ size_t fwd_lds(int NT) const { return (size_t)3 * NT * 16 * P * sizeof(float); }
    // backward: H[0..D], T[0..D-1], R[0..D-2] (the last block's R lives in Gz), G, Gz, U, the observations and dL/dlogits | dL/dv
    __host__ __device__ size_t bwd_lds() const { return (size_t)16 * ((3 * D + 3) * P + XP + A + 1) * sizeof(float); }
    // backward, LEAN (shapes whose saved activations do not fit, e.g. A = 5, Ch = 16, D = 2): H[0..D-1], one T, G, Gz, U -- H_D lives in Gz
    // until the heads are done, relu(conv0) and relu(conv1) of a block are recomputed when the walk back reaches it
    __host__ __device__ size_t bwd_lds_lean() const { return (size_t)16 * ((D + 4) * P + XP + A + 1) * sizeof(float); }

    // ---- the 8 + 8 D tensors of net.parameters(): tensor 4 l + 2 dir = the weight [Ch, Cin, 2A-1] of layer l's row (dir 0) / column
    // (dir 1) convolution, 4 l + 2 dir + 1 its bias [Ch]; 4 L .. 4 L + 3 = policy.weight [A, F], policy.bias, value.weight [F], value.bias
    __host__ __device__ int n_tensors() const { return 4 * L + 4; }
    __host__ __device__ int tensor_size(int j) const {
        if (j < 4 * L) return (j & 1) ? Ch : wsize(j / 4);
        return j == 4 * L ? A * F : j == 4 * L + 1 ? A : j == 4 * L + 2 ? F : 1;
    }
    // element i of the flat bucket (0 <= i < n_params()) -> its tensor; *e: the element inside it
    __host__ __device__ int locate(int i, int *e) const {
        const int b0 = 2 * (wsize(0) + Ch), per = 2 * (wsize(1) + Ch);
        int l, r;
        if (i < b0) { l = 0; r = i; }
        else if (i < b0 + 2 * D * per) { l = 1 + (i - b0) / per; r = (i - b0) % per; }
        else {
            r = i - b0 - 2 * D * per;
            if (r < A * F) { *e = r; return 4 * L; }
            if (r < A * F + A) { *e = r - A * F; return 4 * L + 1; }
            if (r < A * F + A + F) { *e = r - A * F - A; return 4 * L + 2; }
            *e = 0;
            return 4 * L + 3;
        }
        const int ws = wsize(l), dir = r / (ws + Ch);
        r -= dir * (ws + Ch);
        if (r < ws) { *e = r; return 4 * l + 2 * dir; }
        *e = r - ws;
        return 4 * l + 2 * dir + 1;
    }
    // a bias of a CrossConv: its image slot holds row_conv.bias[o] + col_conv.bias[o]
    __host__ __device__ bool is_conv_bias(int j) const { return j < 4 * L && (j & 1); }
};

// The slot of entry (m, k) of a Toeplitz operand image with KSl k-steps: MFMA A-operand order, 64 floats per (m-tile, k-step), lane
// (k & 3) * 16 + (m & 15) (conv_tower.hip, "Operand order").
__host__ __device__ inline int conv_operand_slot(int KSl, int m, int k) { return (m >> 4) * (KSl * 64) + (k >> 2) * 64 + (k & 3) * 16 + (m & 15); }

// emit(slot) for every slot of the packed image that k_conv_pack fills from element e of tensor j -- the inverse of its gather; returns
// their number.  A conv weight W[o, c, t] is the entry ((o, y), (c, x)) of the forward Toeplitz operand for every 0 <= x, y < A with
// x - y + A - 1 == t (A - |t - (A - 1)| of them) and, in the tower layers, the entry ((c, x), (o, y)) of the transposed operand for the
// same (x, y); a conv bias names the slot of the SUM row bias + column bias of its channel (so two elements name it); a head weight
// or bias has one slot.  The K padding of the pre-layer's operands and the tail padding of the image are named by no element.
template <typename Emit>
__host__ __device__ inline int conv_image_slots(const ConvShape &sh, int j, int e, Emit emit) {
    const int A = sh.A, L = sh.L;
    if (j >= 4 * L) {
        emit(j == 4 * L ? sh.wp() + e : j == 4 * L + 1 ? sh.bp() + e : j == 4 * L + 2 ? sh.wv() + e : sh.bv());
        return 1;
    }
    const int l = j / 4, dir = (j / 2) & 1;
    if (j & 1) {
        emit(sh.bias(l) + e);
        return 1;
    }
    const int T = 2 * A - 1, cin = sh.cin(l);
    const int o = e / (cin * T), c = (e / T) % cin, t = e % T;
    const int y0 = t < A - 1 ? A - 1 - t : 0, y1 = t < A - 1 ? A - 1 : 2 * A - 2 - t;
    int n = 0;
    for (int y = y0; y <= y1; ++y) {
        const int x = t + y - (A - 1);
        emit(sh.fwd(l) + dir * sh.image(l) + conv_operand_slot(sh.ks(l), o * A + y, c * A + x));
        ++n;
        if (l >= 1) {
            emit(sh.tr(l) + dir * sh.image(l) + conv_operand_slot(sh.KS, c * A + x, o * A + y));
            ++n;
        }
    }
    return n;
}

}  // namespace rnad
