// Backward of the audio transformer's self-attention (csrc/attention.hip): the shared
// flash-attention-2 backward of attention_backward_core.h over dense [B, S, .] rows read through a row stride, head dim 64,
// the row log-sum-exp L of amav_selfattn_forward_lse and delta as [B, H, S].  Keys and queries are the same S rows.
#include <cmath>

#include "attention_backward_core.h"

namespace amav {
namespace attn_bwd {

constexpr int kD = 64;  // head dim

struct DenseRows {
    const float *q, *k, *v;  // rows of `rs` floats
    long long rs;
    const float *out, *dout;
    long long out_rs, dout_rs;
    const float *lse;
    float *delta;          // [B, H, S]
    float *dq, *dk, *dv;   // rows of `g_rs` floats
    long long g_rs;
    int B, S, H;

    __device__ long long delta_rows() const { return (long long)B * S * H; }
    // pair r = (b * S + i) * H + head: rows in memory order, so the reads are contiguous
    __device__ void delta_io(long long r, const float *&o, const float *&g, float *&d) const {
        const int head = (int)(r % H), i = (int)((r / H) % S), b = (int)(r / ((long long)H * S));
        o = out + ((size_t)b * S + i) * out_rs + head * kD;
        g = dout + ((size_t)b * S + i) * dout_rs + head * kD;
        d = delta + ((size_t)b * H + head) * S + i;
    }
    __device__ void bind(int head, int b) {
        const size_t row = (size_t)b * S, bh = ((size_t)b * H + head) * S;
        q += row * rs + head * kD, k += row * rs + head * kD, v += row * rs + head * kD;
        dout += row * dout_rs + head * kD;
        lse += bh, delta += bh;
        dq += row * g_rs + head * kD, dk += row * g_rs + head * kD, dv += row * g_rs + head * kD;
    }
    __device__ int keys() const { return S; }
    __device__ int queries() const { return S; }
    __device__ const float *q_row(int i) const { return q + (size_t)i * rs; }
    __device__ const float *k_row(int j) const { return k + (size_t)j * rs; }
    __device__ const float *v_row(int j) const { return v + (size_t)j * rs; }
    __device__ const float *dout_row(int i) const { return dout + (size_t)i * dout_rs; }
    __device__ float lse_at(int i) const { return lse[i]; }
    __device__ float delta_at(int i) const { return delta[i]; }
    __device__ float *dq_row(int i) const { return dq + (size_t)i * g_rs; }
    __device__ float *dk_row(int j) const { return dk + (size_t)j * g_rs; }
    __device__ float *dv_row(int j) const { return dv + (size_t)j * g_rs; }
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
    const attn_bwd::DenseRows rows = {q, k, v, row_stride, out, dout, out_row_stride, dout_row_stride, lse, delta,
                                      dqkv, dqkv + hd, dqkv + 2 * hd, dqkv_row_stride, B, S, H};
    constexpr int kD = attn_bwd::kD;
    attn_bwd::delta_kernel<kD><<<blocks_for((long long)B * S * H * (kD / 4)), 256, 0, stream>>>(rows);
    const dim3 grid((unsigned)((S + attn_bwd::kBW - 1) / attn_bwd::kBW), H, B);
    attn_bwd::dkdv_kernel<kD><<<grid, 256, 0, stream>>>(rows, scale);
    attn_bwd::dq_kernel<kD><<<grid, 256, 0, stream>>>(rows, scale);
    return check_launch("amav_selfattn_backward");
}
