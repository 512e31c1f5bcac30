// Dense attention rows: how the backward kernels of attention_backward.hip (fp32 products,
// through attention_backward_core.h's accessors) and attention_backward_split.hip (fp16 x 2 split products, through the
// fields and bind) address [B, S, .] rows of head dim 64, and the argument checks their entry points share.
#pragma once
#include <cmath>

#include "amav_common.h"

namespace amav {
namespace attn_bwd {

constexpr int kD = 64;  // head dim

// Sq query rows (q, out, dout, lse, delta, dq) and Sk key rows (k, v, dk, dv) per batch item, each tensor behind its own
// row stride.  Cross-attention: k | v and dk | dv are the halves of fused [B, Sk, 2*H*64] rows.  Self-attention is the
// same with Sq = Sk = S, q | k | v the thirds of one fused row and dq | dk | dv the thirds of another.
struct DenseRows {
    const float *q;
    long long q_rs;
    const float *k, *v;    // rows of `kv_rs` floats
    long long kv_rs;
    const float *out, *dout;
    long long out_rs, dout_rs;
    const float *lse;
    float *delta;          // [B, H, Sq], in the workspace: set by the launch
    float *dq;
    long long dq_rs;
    float *dk, *dv;        // rows of `dkv_rs` floats
    long long dkv_rs;
    int B, Sq, Sk, H;

    __device__ long long delta_rows() const { return (long long)B * Sq * H; }
    __device__ void delta_io(long long r, const float *&o, const float *&g, float *&d) const {
        const int head = (int)(r % H), i = (int)((r / H) % Sq), b = (int)(r / ((long long)H * Sq));
        o = out + ((size_t)b * Sq + i) * out_rs + head * kD;
        g = dout + ((size_t)b * Sq + i) * dout_rs + head * kD;
        d = delta + ((size_t)b * H + head) * Sq + i;
    }
    __device__ void bind(int head, int b) {
        const size_t qrow = (size_t)b * Sq, krow = (size_t)b * Sk, bh = ((size_t)b * H + head) * Sq;
        q += qrow * q_rs + head * kD, k += krow * kv_rs + head * kD, v += krow * kv_rs + head * kD;
        dout += qrow * dout_rs + head * kD;
        lse += bh, delta += bh;
        dq += qrow * dq_rs + head * kD, dk += krow * dkv_rs + head * kD, dv += krow * dkv_rs + head * kD;
    }
    __device__ int keys() const { return Sk; }
    __device__ int queries() const { return Sq; }
    __device__ const float *q_row(int i) const { return q + (size_t)i * q_rs; }
    __device__ const float *k_row(int j) const { return k + (size_t)j * kv_rs; }
    __device__ const float *v_row(int j) const { return v + (size_t)j * kv_rs; }
    __device__ const float *dout_row(int i) const { return dout + (size_t)i * dout_rs; }
    __device__ float lse_at(int i) const { return lse[i]; }
    __device__ float delta_at(int i) const { return delta[i]; }
    __device__ float *dq_row(int i) const { return dq + (size_t)i * dq_rs; }
    __device__ float *dk_row(int j) const { return dk + (size_t)j * dkv_rs; }
    __device__ float *dv_row(int j) const { return dv + (size_t)j * dkv_rs; }
};

// The refusals every dense backward entry point shares, `what` being its name: sizes, head dim, NULLs, row strides,
// alignment, finite scale, grid limits and a workspace of `need` bytes.  `r.dk` may still be the start of the fused
// gradient rows it lies in and `r.dv` unset: the caller checks what those rows must hold (dqkv / dkv row stride) before,
// and addresses dk and dv in them after.
inline int check_dense_backward(const char *what, const DenseRows &r, int D, float scale, size_t need, const void *workspace,
                                size_t workspace_bytes) {
    AMAV_REQUIRE(r.B > 0 && r.Sq > 0 && r.Sk > 0 && r.H > 0, "%s: bad sizes B=%d Sq=%d Sk=%d H=%d", what, r.B, r.Sq, r.Sk, r.H);
    AMAV_REQUIRE(D == kD, "%s: head_dim %d (only %d is built)", what, D, kD);
    AMAV_REQUIRE(r.q && r.k && r.v && r.out && r.lse && r.dout && r.dq && r.dk, "%s: NULL pointer", what);
    const long long hd = (long long)r.H * D;
    AMAV_REQUIRE(r.q_rs >= hd && r.kv_rs >= hd && r.out_rs >= hd && r.dout_rs >= hd && r.dq_rs >= hd && r.dkv_rs >= hd &&
                     (r.q_rs | r.kv_rs | r.out_rs | r.dout_rs | r.dq_rs | r.dkv_rs) % 4 == 0,
                 "%s: q, k/v, out, dout, dq and dk/dv row strides must be multiples of 4 floats and >= H*D", what);
    AMAV_REQUIRE(aligned16(r.q, r.k, r.v, r.out, r.dout, r.dq, r.dk) && (reinterpret_cast<uintptr_t>(r.lse) & 3) == 0,
                 "%s: q/k/v/out/dout and the gradients must be 16-byte aligned, lse 4-byte aligned", what);
    AMAV_REQUIRE(std::isfinite(scale), "%s: scale must be finite", what);
    AMAV_REQUIRE(r.H <= 65535 && r.B <= 65535, "%s: grid too large", what);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, need);
    return AMAV_OK;
}

}  // namespace attn_bwd
}  // namespace amav
