"""Child process of test_attention_forward_gpu.py: AMAV_ATTN_SPLIT (the forced key split) is read once per process, so
every forced split runs in a fresh process that has not touched the GPU before.

    AMAV_ATTN_SPLIT=n python tests/attention_forced_split_child.py OUT.pt

For every shape of attention_cases.FORCED_SHAPES (unit randn, fused-qkv row stride) and all three variants: selfattn;
for the default variant also selfattn_lse, the split-out operand and split_operand of the fp32 result; and the
workspace size under the f32 variant, from which the parent reads the split that ran.  Everything is saved to OUT.pt;
the comparisons are the parent's."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import attention_cases as ac  # noqa: E402


def main(path):
    from audio_motion_avatar_amd import _lib, ops

    t0 = time.time()
    results = {"forced": os.environ.get("AMAV_ATTN_SPLIT"), "shapes": {}}
    for B, S, H in ac.FORCED_SHAPES:
        case = ac.unit_case(B, S, H)
        HD = H * ac.D
        qkv = torch.cat([case.q, case.k, case.v, torch.zeros(B, S, 12)], dim=-1).cuda()[..., :3 * HD]
        q, k, v = qkv[..., :HD], qkv[..., HD:2 * HD], qkv[..., 2 * HD:]
        rec = {}
        try:
            for variant in ac.VARIANTS:
                ops.set_option("attn", variant)
                rec[variant] = ops.selfattn(q, k, v, H).cpu()
                if variant == "f32":
                    rec["workspace_bytes_f32"] = int(_lib.lib().amav_selfattn_workspace_bytes(B, S, H, ac.D))
        finally:
            ops.set_option("attn", "default")
        out, lse = ops.selfattn_lse(qkv, H)
        rec["lse_out"], rec["lse"] = out.cpu(), lse.cpu()
        rec["split_out"] = ops.selfattn(q, k, v, H, split_out_exp=ac.SPLIT_OUT_EXP).cpu()
        rec["split_want"] = ops.split_operand(ops.selfattn(q, k, v, H).view(-1, HD), fmt=ops.SPLIT_FP16X2,
                                              scale_exp=ac.SPLIT_OUT_EXP).cpu()
        results["shapes"][(B, S, H)] = rec
    torch.cuda.synchronize()
    results["seconds"] = time.time() - t0
    torch.save(results, path)


if __name__ == "__main__":
    main(sys.argv[1])
