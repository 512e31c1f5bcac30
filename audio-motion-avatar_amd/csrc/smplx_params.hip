// The SMPL-X parameter term of the two training steps, for gfx950: the decoder's rot6d -> axis-angle conversion
// (smplx_decoder.py: matrix_to_axis_angle(rotation_6d_to_matrix(d6))) and losses.smplx_param_loss, each as one forward
// and one backward launch.  The arithmetic is a few kFLOP on at most a few thousand rotations; what the launches replace
// is the library's chain of several hundred tiny operators per call.
//
//   rot6d_forward_kernel / rot6d_backward_kernel   one lane per rotation; the backward recomputes the forward from d6
//                    (nothing is saved) and takes every branch from the record rot6d_forward returns (smplx_rotation.h).
//   loss_forward_kernel   blocks of 256 threads walk every present term with a grid stride, one lane per rotation pair
//                    or per element, and keep twelve running sums per lane (in double, like all arithmetic here:
//                    smplx_rotation.h says why).  wave_sum (wave_ops.h), then the four waves
//                    in ascending order.  One workgroup (every training size: F <= 64 frames is at most 1344 rows per
//                    term) divides by the counts and writes parts [12] itself; more workgroups write their twelve sums
//                    to their own workspace slot, and loss_finalize_kernel adds the slots in ascending order.  No float
//                    atomics: the same bits on every run.
//   loss_backward_kernel  the same walk; every gradient element is written exactly once by the lane that owns it, with
//                    the gates (clamp, sign(0) = 0, |d| < 1) replayed from the forward's functions.
#include <climits>
#include <cstddef>

#include "amav_common.h"
#include "smplx_rotation.h"
#include "wave_ops.h"

namespace amav {
namespace smplx {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kTerms = AMAV_SMPLX_TERMS;     // betas, the seven rotation keys, expression, transl
constexpr int kParts = AMAV_SMPLX_PARTS;     // betas_mse, betas_prior, seven *_geo, expression_l1, expression_prior, transl
constexpr int kRotFirst = 1, kRotCount = 7;  // terms 1..7 hold rows of three floats; their parts are 2..8
constexpr int kBetas = 0, kExpression = 8, kTransl = 9;
constexpr int kItemsPerBlock = 4096;         // 16 items per lane and term before a second workgroup is worth its slot
constexpr int kMaxBlocks = 256;

__global__ __launch_bounds__(kBlock) void rot6d_forward_kernel(int n, const float *__restrict__ d6, int64_t row_stride,
                                                               float *__restrict__ aa) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    real x[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) x[a] = d6[(int64_t)i * row_stride + a];
    const Rot6d r = rot6d_forward(x);
#pragma unroll
    for (int a = 0; a < 3; ++a) aa[(int64_t)i * 3 + a] = (float)r.aa[a];
}

__global__ __launch_bounds__(kBlock) void rot6d_backward_kernel(int n, const float *__restrict__ d6, int64_t row_stride,
                                                                const float *__restrict__ grad_aa,
                                                                float *__restrict__ grad_d6) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    real x[6], g[3], gx[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) x[a] = d6[(int64_t)i * row_stride + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = grad_aa[(int64_t)i * 3 + a];
    const Rot6d r = rot6d_forward(x);
    rot6d_backward(x, r, g, gx);
#pragma unroll
    for (int a = 0; a < 6; ++a) grad_d6[(int64_t)i * 6 + a] = (float)gx[a];
}

__device__ __forceinline__ bool present(const amav_smplx_term &t) { return t.pred != nullptr && t.frames > 0 && t.per_frame > 0; }
__device__ __forceinline__ int items_of(const amav_smplx_term &t) { return present(t) ? t.frames * t.per_frame : 0; }

// item i of a term -> offsets of its first float in pred and gt; `width` floats per item (3 for a rotation row)
struct At {
    int64_t pred, gt;
};
__device__ __forceinline__ At locate(const amav_smplx_term &t, int i, int width) {
    const int f = i / t.per_frame, j = i - f * t.per_frame;
    return {(int64_t)f * t.pred_stride + (int64_t)j * width, (int64_t)f * t.gt_stride + (int64_t)j * width};
}

__device__ __forceinline__ real sign_of(real d) { return (real)(d > 0.0) - (real)(d < 0.0); }  // sign(0) = 0
__device__ __forceinline__ real smooth_l1(real d) {  // beta = 1
    const real a = fabs(d);
    return a < 1.0 ? 0.5 * d * d : a - 0.5;
}
__device__ __forceinline__ real smooth_l1_grad(real d) { return fabs(d) < 1.0 ? d : sign_of(d); }

// what a part's sum is divided by: the elements (or rotation rows) of its term
__device__ __forceinline__ int part_term(int part) {
    return part < 2 ? kBetas : part < 2 + kRotCount ? kRotFirst + part - 2 : part < 11 ? kExpression : kTransl;
}

// out: parts [12] (fp32) with kFinal (one workgroup), else this workgroup's slot of [gridDim.x, 12] sums (real)
template <bool kFinal>
__global__ __launch_bounds__(kBlock) void loss_forward_kernel(amav_smplx_terms terms, void *__restrict__ out) {
    __shared__ real wave_sums[kParts][kWaves];
    const int first = blockIdx.x * kBlock + threadIdx.x, step = gridDim.x * kBlock;
    real acc[kParts];
#pragma unroll
    for (int p = 0; p < kParts; ++p) acc[p] = 0.0;

    {
        const amav_smplx_term &t = terms.term[kBetas];
        for (int i = first, n = items_of(t); i < n; i += step) {
            const At at = locate(t, i, 1);
            const real p = t.pred[at.pred], d = p - (real)t.gt[at.gt];
            acc[0] += d * d;
            acc[1] += p * p;
        }
    }
#pragma unroll
    for (int k = 0; k < kRotCount; ++k) {
        const amav_smplx_term &t = terms.term[kRotFirst + k];
        for (int i = first, n = items_of(t); i < n; i += step) {
            const At at = locate(t, i, 3);
            const real rp[3] = {t.pred[at.pred], t.pred[at.pred + 1], t.pred[at.pred + 2]};
            const real rg[3] = {t.gt[at.gt], t.gt[at.gt + 1], t.gt[at.gt + 2]};
            acc[2 + k] += geodesic_forward(rp, rg).value;
        }
    }
    {
        const amav_smplx_term &t = terms.term[kExpression];
        for (int i = first, n = items_of(t); i < n; i += step) {
            const At at = locate(t, i, 1);
            const real p = t.pred[at.pred];
            acc[9] += fabs(p - (real)t.gt[at.gt]);
            acc[10] += p * p;
        }
    }
    {
        const amav_smplx_term &t = terms.term[kTransl];
        for (int i = first, n = items_of(t); i < n; i += step) {
            const At at = locate(t, i, 1);
            acc[11] += smooth_l1((real)t.pred[at.pred] - (real)t.gt[at.gt]);
        }
    }

    // fixed order: the xor butterfly inside each wave, then the waves in ascending order
#pragma unroll
    for (int p = 0; p < kParts; ++p) {
        const real s = wave_sum(acc[p]);
        if (threadIdx.x % kWave == 0) wave_sums[p][threadIdx.x / kWave] = s;
    }
    __syncthreads();
    if (threadIdx.x < kParts) {
        const int p = threadIdx.x;
        real s = 0.0;
        for (int w = 0; w < kWaves; ++w) s += wave_sums[p][w];
        if (kFinal) {
            const int n = items_of(terms.term[part_term(p)]);
            static_cast<float *>(out)[p] = n > 0 ? (float)(s / n) : 0.0f;
        } else {
            static_cast<real *>(out)[(int64_t)blockIdx.x * kParts + p] = s;
        }
    }
}

// one wave: lane p adds part p's slots in ascending order
__global__ __launch_bounds__(kWave) void loss_finalize_kernel(amav_smplx_terms terms, int slots,
                                                              const real *__restrict__ partial,
                                                              float *__restrict__ parts) {
    const int p = threadIdx.x;
    if (p >= kParts) return;
    real s = 0.0;
    for (int b = 0; b < slots; ++b) s += partial[(int64_t)b * kParts + p];
    const int n = items_of(terms.term[part_term(p)]);
    parts[p] = n > 0 ? (float)(s / n) : 0.0f;
}

// grads.grad[k]: NULL, or [frames, per_frame (x 3)] contiguous; grad_parts [12] on the device
__global__ __launch_bounds__(kBlock) void loss_backward_kernel(amav_smplx_terms terms, amav_smplx_grads grads,
                                                               const float *__restrict__ grad_parts) {
    const int first = blockIdx.x * kBlock + threadIdx.x, step = gridDim.x * kBlock;
    if (grads.grad[kBetas]) {
        const amav_smplx_term &t = terms.term[kBetas];
        const int n = items_of(t);
        const real g_mse = (real)grad_parts[0] / n, g_prior = (real)grad_parts[1] / n;
        for (int i = first; i < n; i += step) {
            const At at = locate(t, i, 1);
            const real p = t.pred[at.pred], d = p - (real)t.gt[at.gt];
            grads.grad[kBetas][i] = (float)(g_mse * 2.0 * d + g_prior * 2.0 * p);
        }
    }
#pragma unroll
    for (int k = 0; k < kRotCount; ++k) {
        float *out = grads.grad[kRotFirst + k];
        if (!out) continue;
        const amav_smplx_term &t = terms.term[kRotFirst + k];
        const int n = items_of(t);
        const real g = (real)grad_parts[2 + k] / n;
        for (int i = first; i < n; i += step) {
            const At at = locate(t, i, 3);
            const real rp[3] = {t.pred[at.pred], t.pred[at.pred + 1], t.pred[at.pred + 2]};
            const real rg[3] = {t.gt[at.gt], t.gt[at.gt + 1], t.gt[at.gt + 2]};
            real grp[3];
            geodesic_backward(rp, geodesic_forward(rp, rg), g, grp);
#pragma unroll
            for (int a = 0; a < 3; ++a) out[(int64_t)i * 3 + a] = (float)grp[a];
        }
    }
    if (grads.grad[kExpression]) {
        const amav_smplx_term &t = terms.term[kExpression];
        const int n = items_of(t);
        const real g_l1 = (real)grad_parts[9] / n, g_prior = (real)grad_parts[10] / n;
        for (int i = first; i < n; i += step) {
            const At at = locate(t, i, 1);
            const real p = t.pred[at.pred], d = p - (real)t.gt[at.gt];
            grads.grad[kExpression][i] = (float)(g_l1 * sign_of(d) + g_prior * 2.0 * p);
        }
    }
    if (grads.grad[kTransl]) {
        const amav_smplx_term &t = terms.term[kTransl];
        const int n = items_of(t);
        const real g = (real)grad_parts[11] / n;
        for (int i = first; i < n; i += step) {
            const At at = locate(t, i, 1);
            grads.grad[kTransl][i] = (float)(g * smooth_l1_grad((real)t.pred[at.pred] - (real)t.gt[at.gt]));
        }
    }
}

// host: a term is present when it has a pointer; the launch sees the same rule (present())
inline bool given(const amav_smplx_term &t) { return t.pred != nullptr || t.gt != nullptr; }

// the checks the loss entry points share; *largest receives the most items any term has
inline int check_terms(const char *what, const amav_smplx_terms *terms, int *largest) {
    AMAV_REQUIRE(terms, "%s: NULL pointer (terms)", what);
    *largest = 0;
    for (int k = 0; k < kTerms; ++k) {
        const amav_smplx_term &t = terms->term[k];
        AMAV_REQUIRE(t.frames >= 0 && t.per_frame >= 0, "%s: negative count in term %d (frames=%d per_frame=%d)", what, k,
                     t.frames, t.per_frame);
        if (!given(t) || t.frames == 0 || t.per_frame == 0) continue;
        AMAV_REQUIRE(t.pred && t.gt, "%s: NULL pointer in term %d (pred / gt of a present term)", what, k);
        const int width = k >= kRotFirst && k < kRotFirst + kRotCount ? 3 : 1;
        const int64_t items = (int64_t)t.frames * t.per_frame;
        // half the int range: the kernels' grid-stride index steps past the last item before it stops
        AMAV_REQUIRE(items * width <= INT_MAX / 2, "%s: term %d exceeds 2^30 - 1 floats (frames=%d per_frame=%d)", what, k,
                     t.frames, t.per_frame);
        if (items > *largest) *largest = (int)items;
    }
    return AMAV_OK;
}

inline int blocks_of(int largest) {
    const int b = (largest + kItemsPerBlock - 1) / kItemsPerBlock;
    return b < 1 ? 1 : b > kMaxBlocks ? kMaxBlocks : b;
}

// a term without its pointers is absent for the kernels whatever its counts say
inline amav_smplx_terms launchable(const amav_smplx_terms &in) {
    amav_smplx_terms t = in;
    for (int k = 0; k < kTerms; ++k)
        if (!t.term[k].pred || !t.term[k].gt) t.term[k] = amav_smplx_term{nullptr, nullptr, 0, 0, 0, 0};
    return t;
}

inline int check_rows(const char *what, int n) {
    AMAV_REQUIRE(n >= 0, "%s: negative count n=%d", what, n);
    AMAV_REQUIRE(n <= INT_MAX / 6, "%s: n=%d exceeds 2^31 - 1 floats", what, n);
    return AMAV_OK;
}

}  // namespace smplx
}  // namespace amav

using namespace amav;
using namespace amav::smplx;

extern "C" int amav_rot6d_to_axis_angle(int n, const float *d6_dev, int64_t row_stride, float *aa_dev, void *stream_) {
    if (int rc = check_rows("amav_rot6d_to_axis_angle", n)) return rc;
    if (n == 0) return AMAV_OK;  // an empty problem
    AMAV_REQUIRE(d6_dev && aa_dev, "amav_rot6d_to_axis_angle: NULL pointer (d6 / aa)");
    rot6d_forward_kernel<<<blocks_for(n), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(n, d6_dev, row_stride, aa_dev);
    return check_launch("amav_rot6d_to_axis_angle: rot6d_forward_kernel");
}

extern "C" int amav_rot6d_to_axis_angle_backward(int n, const float *d6_dev, int64_t row_stride, const float *grad_aa_dev,
                                                 float *grad_d6_dev, void *stream_) {
    if (int rc = check_rows("amav_rot6d_to_axis_angle_backward", n)) return rc;
    if (n == 0) return AMAV_OK;  // an empty gradient
    AMAV_REQUIRE(d6_dev && grad_aa_dev && grad_d6_dev, "amav_rot6d_to_axis_angle_backward: NULL pointer (d6 / grad_aa / grad_d6)");
    rot6d_backward_kernel<<<blocks_for(n), kBlock, 0, static_cast<hipStream_t>(stream_)>>>(n, d6_dev, row_stride,
                                                                                          grad_aa_dev, grad_d6_dev);
    return check_launch("amav_rot6d_to_axis_angle_backward: rot6d_backward_kernel");
}

extern "C" size_t amav_smplx_param_loss_workspace_bytes(const amav_smplx_terms *terms) {
    int largest = 0;
    if (check_terms("amav_smplx_param_loss_workspace_bytes", terms, &largest)) return 0;
    const int blocks = blocks_of(largest);
    return blocks > 1 ? (size_t)blocks * kParts * sizeof(real) : 0;
}

extern "C" int amav_smplx_param_loss_forward(const amav_smplx_terms *terms, float *parts_dev, void *workspace_dev,
                                             size_t workspace_bytes, void *stream_) {
    int largest = 0;
    if (int rc = check_terms("amav_smplx_param_loss_forward", terms, &largest)) return rc;
    AMAV_REQUIRE(parts_dev, "amav_smplx_param_loss_forward: NULL pointer (parts)");
    const int blocks = blocks_of(largest);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const amav_smplx_terms t = launchable(*terms);
    if (blocks == 1) {
        loss_forward_kernel<true><<<1, kBlock, 0, stream>>>(t, parts_dev);
        return check_launch("amav_smplx_param_loss_forward: loss_forward_kernel");
    }
    const size_t need = (size_t)blocks * kParts * sizeof(real);
    if (int rc = check_workspace("amav_smplx_param_loss_forward", need, workspace_dev, workspace_bytes)) return rc;
    real *partial = static_cast<real *>(workspace_dev);
    loss_forward_kernel<false><<<(unsigned)blocks, kBlock, 0, stream>>>(t, partial);
    if (int rc = check_launch("amav_smplx_param_loss_forward: loss_forward_kernel")) return rc;
    loss_finalize_kernel<<<1, kWave, 0, stream>>>(t, blocks, partial, parts_dev);
    return check_launch("amav_smplx_param_loss_forward: loss_finalize_kernel");
}

extern "C" int amav_smplx_param_loss_backward(const amav_smplx_terms *terms, const float *grad_parts_dev,
                                              const amav_smplx_grads *grads, void *stream_) {
    int largest = 0;
    if (int rc = check_terms("amav_smplx_param_loss_backward", terms, &largest)) return rc;
    AMAV_REQUIRE(grads, "amav_smplx_param_loss_backward: NULL pointer (grads)");
    const amav_smplx_terms t = launchable(*terms);
    amav_smplx_grads g = *grads;
    bool any = false;
    for (int k = 0; k < kTerms; ++k) {
        if (!t.term[k].pred || t.term[k].frames == 0 || t.term[k].per_frame == 0) g.grad[k] = nullptr;  // nothing to write
        any = any || g.grad[k];
    }
    if (!any) return AMAV_OK;
    AMAV_REQUIRE(grad_parts_dev, "amav_smplx_param_loss_backward: NULL pointer (grad_parts)");
    const int blocks = (largest + kBlock - 1) / kBlock;
    loss_backward_kernel<<<(unsigned)(blocks < kMaxBlocks * 16 ? blocks : kMaxBlocks * 16), kBlock, 0,
                           static_cast<hipStream_t>(stream_)>>>(t, g, grad_parts_dev);
    return check_launch("amav_smplx_param_loss_backward: loss_backward_kernel");
}
