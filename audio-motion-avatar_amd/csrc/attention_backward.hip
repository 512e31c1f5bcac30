// Backward of the audio transformer's self-attention (csrc/attention.hip): the shared
// flash-attention-2 backward of attention_backward_core.h over dense [B, S, .] rows read through a row stride
// (attention_dense_rows.h), head dim 64, the row log-sum-exp L of the forward and delta as [B, H, Sq].  Keys and queries
// are the same S rows (the audio net's self-attention) or, for the stage-1 encoder's cross-attention, Sq query rows over
// Sk key rows.
#include "attention_backward_core.h"
#include "attention_dense_rows.h"

namespace amav {
namespace attn_bwd {

static size_t workspace_bytes(int B, int Sq, int H) { return align_up((size_t)B * H * Sq * sizeof(float), 256); }  // delta

// `rows.delta` is set here; three kernels, no host synchronisation
static int launch(DenseRows rows, float scale, void *workspace, hipStream_t stream, const char *what) {
    rows.delta = static_cast<float *>(workspace);
    delta_kernel<kD><<<blocks_for((long long)rows.B * rows.Sq * rows.H * (kD / 4)), 256, 0, stream>>>(rows);
    const dim3 key_grid((unsigned)((rows.Sk + kBW - 1) / kBW), rows.H, rows.B);
    const dim3 query_grid((unsigned)((rows.Sq + kBW - 1) / kBW), rows.H, rows.B);
    dkdv_kernel<kD><<<key_grid, 256, 0, stream>>>(rows, scale);
    dq_kernel<kD><<<query_grid, 256, 0, stream>>>(rows, scale);
    return check_launch(what);
}

}  // namespace attn_bwd
}  // namespace amav

using namespace amav;

extern "C" size_t amav_selfattn_backward_workspace_bytes(int B, int S, int H, int D) {
    if (B <= 0 || S <= 0 || H <= 0 || D != attn_bwd::kD) return 0;
    return attn_bwd::workspace_bytes(B, S, H);
}

extern "C" int amav_selfattn_backward(int B, int S, int H, int D, const float *q, const float *k, const float *v,
                                      int64_t row_stride, const float *out, int64_t out_row_stride, const float *lse,
                                      const float *dout, int64_t dout_row_stride, float *dqkv, int64_t dqkv_row_stride,
                                      float scale, void *workspace, size_t workspace_bytes, void *stream_) {
    const char *what = "amav_selfattn_backward";
    const int64_t hd = (int64_t)H * attn_bwd::kD;  // D itself is checked with the rest
    AMAV_REQUIRE(dqkv_row_stride >= 3 * hd && dqkv_row_stride % 4 == 0,
                 "%s: dqkv row stride must be a multiple of 4 floats and >= 3*H*D", what);
    attn_bwd::DenseRows rows = {q, row_stride, k, v, row_stride, out, dout, out_row_stride, dout_row_stride, lse, nullptr,
                                dqkv, dqkv_row_stride, dqkv, nullptr, dqkv_row_stride, B, S, S, H};
    if (int rc = attn_bwd::check_dense_backward(what, rows, D, scale, amav_selfattn_backward_workspace_bytes(B, S, H, D),
                                                workspace, workspace_bytes))
        return rc;
    rows.dk = dqkv + hd, rows.dv = dqkv + 2 * hd;
    return attn_bwd::launch(rows, scale, workspace, static_cast<hipStream_t>(stream_), what);
}

extern "C" size_t amav_crossattn_backward_workspace_bytes(int B, int Sq, int H, int D) {
    if (B <= 0 || Sq <= 0 || H <= 0 || D != attn_bwd::kD) return 0;
    return attn_bwd::workspace_bytes(B, Sq, H);
}

extern "C" int amav_crossattn_backward(int B, int Sq, int Sk, int H, int D, const float *q, int64_t q_row_stride,
                                       const float *k, const float *v, int64_t kv_row_stride, const float *out,
                                       int64_t out_row_stride, const float *lse, const float *dout,
                                       int64_t dout_row_stride, float *dq, int64_t dq_row_stride, float *dkv,
                                       int64_t dkv_row_stride, float scale, void *workspace, size_t workspace_bytes,
                                       void *stream_) {
    const char *what = "amav_crossattn_backward";
    const int64_t hd = (int64_t)H * attn_bwd::kD;  // D itself is checked with the rest
    AMAV_REQUIRE(dkv_row_stride >= 2 * hd && dkv_row_stride % 4 == 0,
                 "%s: dkv row stride must be a multiple of 4 floats and >= 2*H*D", what);
    attn_bwd::DenseRows rows = {q, q_row_stride, k, v, kv_row_stride, out, dout, out_row_stride, dout_row_stride, lse, nullptr,
                                dq, dq_row_stride, dkv, nullptr, dkv_row_stride, B, Sq, Sk, H};
    if (int rc = attn_bwd::check_dense_backward(what, rows, D, scale, amav_crossattn_backward_workspace_bytes(B, Sq, H, D),
                                                workspace, workspace_bytes))
        return rc;
    rows.dv = dkv + hd;
    return attn_bwd::launch(rows, scale, workspace, static_cast<hipStream_t>(stream_), what);
}
