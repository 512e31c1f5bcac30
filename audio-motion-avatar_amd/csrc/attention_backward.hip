// Backward of the audio transformer's self-attention (csrc/attention.hip): the shared
// flash-attention-2 backward of attention_backward_core.h over dense [B, S, .] rows read through a row stride, head dim 64,
// the row log-sum-exp L of the forward and delta as [B, H, Sq].  Keys and queries are the same S rows (the audio net's
// self-attention) or, for the stage-1 encoder's cross-attention, Sq query rows over Sk key rows.
#include <cmath>

#include "attention_backward_core.h"

namespace amav {
namespace attn_bwd {

constexpr int kD = 64;  // head dim

// Sq query rows (q, out, dout, lse, delta, dq) and Sk key rows (k, v, dk, dv) per batch item, each tensor behind its own
// row stride.  Self-attention: Sq = Sk = S and one stride for q, k, v and one for dq, dk, dv (thirds of fused rows);
// cross-attention: k | v and dk | dv are the halves of fused [B, Sk, 2*H*64] rows.
struct DenseRows {
    const float *q;
    long long q_rs;
    const float *k, *v;    // rows of `kv_rs` floats
    long long kv_rs;
    const float *out, *dout;
    long long out_rs, dout_rs;
    const float *lse;
    float *delta;          // [B, H, Sq]
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

}  // namespace attn_bwd
}  // namespace amav

using namespace amav;

extern "C" size_t amav_selfattn_backward_workspace_bytes(int B, int S, int H, int D) {
    if (B <= 0 || S <= 0 || H <= 0 || D != attn_bwd::kD) return 0;
    return align_up((size_t)B * H * S * sizeof(float), 256);  // delta [B, H, S]
}

extern "C" int amav_selfattn_backward(int B, int S, int H, int D, const float *q, const float *k, const float *v,
                                      int64_t row_stride, const float *out, int64_t out_row_stride, const float *lse,
                                      const float *dout, int64_t dout_row_stride, float *dqkv, int64_t dqkv_row_stride,
                                      float scale, void *workspace, size_t workspace_bytes, void *stream_) {
    AMAV_REQUIRE(B > 0 && S > 0 && H > 0, "amav_selfattn_backward: bad sizes B=%d S=%d H=%d", B, S, H);
    AMAV_REQUIRE(D == attn_bwd::kD, "amav_selfattn_backward: head_dim %d (only %d is built)", D, attn_bwd::kD);
    AMAV_REQUIRE(q && k && v && out && lse && dout && dqkv, "amav_selfattn_backward: NULL pointer");
    const int64_t hd = (int64_t)H * D;
    AMAV_REQUIRE(row_stride >= hd && out_row_stride >= hd && dout_row_stride >= hd && row_stride % 4 == 0 &&
                     out_row_stride % 4 == 0 && dout_row_stride % 4 == 0,
                 "amav_selfattn_backward: q/k/v, out and dout row strides must be multiples of 4 floats and >= H*D");
    AMAV_REQUIRE(dqkv_row_stride >= 3 * hd && dqkv_row_stride % 4 == 0,
                 "amav_selfattn_backward: dqkv row stride must be a multiple of 4 floats and >= 3*H*D");
    AMAV_REQUIRE(aligned16(q, k, v, out, dout, dqkv) && (reinterpret_cast<uintptr_t>(lse) & 3) == 0,
                 "amav_selfattn_backward: q/k/v/out/dout/dqkv must be 16-byte aligned, lse 4-byte aligned");
    AMAV_REQUIRE(std::isfinite(scale), "amav_selfattn_backward: scale must be finite");
    AMAV_REQUIRE(H <= 65535 && B <= 65535, "amav_selfattn_backward: grid too large");
    const size_t need = amav_selfattn_backward_workspace_bytes(B, S, H, D);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_selfattn_backward: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *delta = static_cast<float *>(workspace);
    const attn_bwd::DenseRows rows = {q, row_stride, k, v, row_stride, out, dout, out_row_stride, dout_row_stride, lse, delta,
                                      dqkv, dqkv_row_stride, dqkv + hd, dqkv + 2 * hd, dqkv_row_stride, B, S, S, H};
    constexpr int kD = attn_bwd::kD;
    attn_bwd::delta_kernel<kD><<<blocks_for((long long)B * S * H * (kD / 4)), 256, 0, stream>>>(rows);
    const dim3 grid((unsigned)((S + attn_bwd::kBW - 1) / attn_bwd::kBW), H, B);
    attn_bwd::dkdv_kernel<kD><<<grid, 256, 0, stream>>>(rows, scale);
    attn_bwd::dq_kernel<kD><<<grid, 256, 0, stream>>>(rows, scale);
    return check_launch("amav_selfattn_backward");
}

extern "C" size_t amav_crossattn_backward_workspace_bytes(int B, int Sq, int H, int D) {
    if (B <= 0 || Sq <= 0 || H <= 0 || D != attn_bwd::kD) return 0;
    return align_up((size_t)B * H * Sq * sizeof(float), 256);  // delta [B, H, Sq]
}

extern "C" int amav_crossattn_backward(int B, int Sq, int Sk, int H, int D, const float *q, int64_t q_row_stride,
                                       const float *k, const float *v, int64_t kv_row_stride, const float *out,
                                       int64_t out_row_stride, const float *lse, const float *dout,
                                       int64_t dout_row_stride, float *dq, int64_t dq_row_stride, float *dkv,
                                       int64_t dkv_row_stride, float scale, void *workspace, size_t workspace_bytes,
                                       void *stream_) {
    AMAV_REQUIRE(B > 0 && Sq > 0 && Sk > 0 && H > 0, "amav_crossattn_backward: bad sizes B=%d Sq=%d Sk=%d H=%d", B, Sq, Sk, H);
    AMAV_REQUIRE(D == attn_bwd::kD, "amav_crossattn_backward: head_dim %d (only %d is built)", D, attn_bwd::kD);
    AMAV_REQUIRE(q && k && v && out && lse && dout && dq && dkv, "amav_crossattn_backward: NULL pointer");
    const int64_t hd = (int64_t)H * D;
    AMAV_REQUIRE(q_row_stride >= hd && kv_row_stride >= hd && out_row_stride >= hd && dout_row_stride >= hd &&
                     dq_row_stride >= hd && q_row_stride % 4 == 0 && kv_row_stride % 4 == 0 && out_row_stride % 4 == 0 &&
                     dout_row_stride % 4 == 0 && dq_row_stride % 4 == 0,
                 "amav_crossattn_backward: q, k/v, out, dout and dq row strides must be multiples of 4 floats and >= H*D");
    AMAV_REQUIRE(dkv_row_stride >= 2 * hd && dkv_row_stride % 4 == 0,
                 "amav_crossattn_backward: dkv row stride must be a multiple of 4 floats and >= 2*H*D");
    AMAV_REQUIRE(aligned16(q, k, v, out, dout, dq, dkv) && (reinterpret_cast<uintptr_t>(lse) & 3) == 0,
                 "amav_crossattn_backward: q/k/v/out/dout/dq/dkv must be 16-byte aligned, lse 4-byte aligned");
    AMAV_REQUIRE(std::isfinite(scale), "amav_crossattn_backward: scale must be finite");
    AMAV_REQUIRE(H <= 65535 && B <= 65535, "amav_crossattn_backward: grid too large");
    const size_t need = amav_crossattn_backward_workspace_bytes(B, Sq, H, D);
    if (workspace == nullptr || workspace_bytes < need)
        return fail(AMAV_ERR_WORKSPACE, "amav_crossattn_backward: workspace %zu < required %zu", workspace_bytes, need);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *delta = static_cast<float *>(workspace);
    const attn_bwd::DenseRows rows = {q, q_row_stride, k, v, kv_row_stride, out, dout, out_row_stride, dout_row_stride,
                                      lse, delta, dq, dq_row_stride, dkv, dkv + hd, dkv_row_stride, B, Sq, Sk, H};
    constexpr int kD = attn_bwd::kD;
    attn_bwd::delta_kernel<kD><<<blocks_for((long long)B * Sq * H * (kD / 4)), 256, 0, stream>>>(rows);
    const dim3 key_grid((unsigned)((Sk + attn_bwd::kBW - 1) / attn_bwd::kBW), H, B);
    const dim3 query_grid((unsigned)((Sq + attn_bwd::kBW - 1) / attn_bwd::kBW), H, B);
    attn_bwd::dkdv_kernel<kD><<<key_grid, 256, 0, stream>>>(rows, scale);
    attn_bwd::dq_kernel<kD><<<query_grid, 256, 0, stream>>>(rows, scale);
    return check_launch("amav_crossattn_backward");
}
