// Types, constants and host helpers shared by lbs.hip (the SMPL-X forward) and lbs_backward.hip (its backward), which
// must read the tables and the pose / coefficient parts exactly as the forward does.
#pragma once
#include "amav_common.h"

namespace amav {
namespace lbs {

constexpr int kMaxJoints = 64;

struct Tables {
    int V, J, NC, KW, KB;  // KB = NC + (J-1)*9 blend rows
    const float *v_template, *blend, *j_template, *j_dirs;
    const int *parents, *skin_idx;
    const float *skin_w;
    const void *blend_split;  // fp16 x 2 form of `blend` (amav_lbs_prepare_blend_split) or NULL
};

constexpr int kMaxFeatures = 64 + (kMaxJoints - 1) * 9;  // KB <= num_coeffs + (J - 1) * 9

// Where the pose and the shape / expression coefficients of a frame come from: the keyword arguments of the SMPL-X
// call as the caller holds them (global_orient, body_pose, jaw_pose, ... / betas, expression: renderer.py:261-272),
// concatenated on load -- smplx's torch.cat + `full_pose += pose_mean` + torch.cat were three launches of ~16 us each
// in front of a 12 us kernel.  One part each = an assembled full_pose / coefficient matrix.
struct PoseSource {
    int nparts, ncparts;
    int first[8], cfirst[4];        // first joint / coefficient of every part
    const float *part[8], *cpart[4];
    long long stride[8], cstride[4];  // floats between frames
    const float *mean;              // [J*3] added to the concatenated pose, or NULL
};

constexpr int kMfmaWaves = 4;                    // frame tiles (of 32) per block
constexpr int kMfmaKC = 32;                      // table rows per staged chunk
constexpr int kMfmaChunk4 = kMfmaKC * 96 / 4;    // float4 per chunk (768)
constexpr int kMfmaKPad = 2 * kMfmaKC;           // zero rows appended to featT on this path

// Host side (lbs.hip).  validate_tables / pose_source return AMAV_OK or an error code with the message set; `who`
// prefixes the message.
int validate_tables(const amav_body_tables *t, const char *who);
Tables make_tables(const amav_body_tables *tb);
int pose_source(const amav_pose_parts *pp, const amav_body_tables *tb, PoseSource *src, const char *who);
// joint_chain_kernel<false>: featT [KB][Fpad] (frames < F only) and A [F][J][12]
void launch_joint_chain(const Tables &t, int F, int Fpad, const PoseSource &src, float *featT, float *A,
                        hipStream_t stream);

}  // namespace lbs
}  // namespace amav
