#!/usr/bin/env python3
"""Golden vectors for stage 1 with `upsample_triplane`, produced by RUNNING THE REFERENCE'S OWN PYTHON on the CPU of the
build container, like tests/golden/make_reference_golden.py -- which this generator imports as a module for its
placeholder machinery (absent third-party packages become inert placeholders; any use of one while fixture data is
produced raises), its name-seeded tensors, its run-phase "zero placeholder uses" assertion and, for the second fixture,
its ToyBody, stage1_cfg and injections.  That generator, its fixtures and ref_manifest.json are left untouched; this
one writes ref_downsampler_manifest.json beside its two fixtures.  Nothing of the reference travels: the fixtures hold
inputs, seeds, parameter names / shapes and outputs only.

  ref_stage1_downsampler.npz  tier 1  TriplaneDownsampler and ConvNeXtBlock exactly as shipped, through their own
                              constructors, in eval mode (src/models/triplane_net.py:411-451): C = 64, 12 x 12 planes,
                              upsample_factor 3, batch 2.  Input, the planes after each block, the output.
  ref_stage1_upsampled.npz    tier 2  SMPLXTriplaneEncoder.__init__/forward (:66-207) with upsample_triplane=True,
                              upsample_factor=3 and the stand-ins of ref_stage1 (smplx.SMPLX := ToyBody, torch_scatter :=
                              oracle/triplane_net.py, diffusers Attention := OracleAttention, pytorch3d rotations :=
                              oracle/rotation.py), B = 2, T = 1 (the reference's .squeeze(1) needs T = 1), ground-truth
                              SMPL-X parameters.  The geometry planes, and the (3R)^2 planes the reference hands to its
                              downsampler (recorded by a forward pre-hook): the only pin of the 3x-resolution cell indexing.

Parameters are not stored: every state_dict entry is seeded_tensor(name, shape) of the base generator.

Run:  python tests/golden/make_downsampler_golden.py      (needs the reference checkout; CPU only)
"""
import importlib
import importlib.util
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SMPL_DIMS = dict(global_orient=3, body_pose=63, betas=10, left_hand_pose=45, right_hand_pose=45, jaw_pose=3, leye_pose=3,
                 reye_pose=3, expression=10, transl=3)


def base_generator():
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(HERE, "make_reference_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # defines functions only
    return mod


def smpl_params_gt(gen, batch, seed=92, scale=0.3):
    """Ground-truth SMPL-X parameters [B,1,dim] from seeds (shared with the tests)."""
    return {k: gen.rnd(seed + i, batch, 1, d, scale=scale) for i, (k, d) in enumerate(SMPL_DIMS.items())}


def fixture_downsampler(gen, tn):
    cfg = types.SimpleNamespace(triplane_feature_dim=64, upsample_factor=3)
    ds = tn.TriplaneDownsampler(cfg).eval()
    assert isinstance(ds.blocks[0], tn.ConvNeXtBlock)
    shapes = {k: list(v.shape) for k, v in ds.state_dict().items()}
    ds.load_state_dict({k: gen.seeded_tensor("triplane_downsampler." + k, v.shape) for k, v in ds.state_dict().items()})
    x = gen.rnd(91, 2, 3, 64, 12, 12)
    with torch.no_grad():
        after = [[], []]
        for i in range(3):
            plane = x[:, i]
            for b, blk in enumerate(ds.blocks):
                plane = blk(plane)
                after[b].append(plane)
        y = ds(x)
    return gen.save("stage1_downsampler", 1, ["src/models/triplane_net.py:411-451"],
                    dict(x=x, after_block0=torch.stack(after[0], dim=1), after_block1=torch.stack(after[1], dim=1), y=y),
                    meta=dict(cfg=vars(cfg), params=shapes, param_prefix="triplane_downsampler."))


def fixture_upsampled(gen, tn, tr, sd_mod):
    sys.path.insert(0, ROOT)
    from oracle import rotation as orot, triplane_net as o_tn

    cfg = gen.stage1_cfg()
    cfg.upsample_triplane, cfg.upsample_factor, cfg.triplane_feature_dim = True, 3, 64
    tr.Attention = gen.OracleAttention
    sd_mod.rotation_6d_to_matrix, sd_mod.matrix_to_axis_angle = orot.rotation_6d_to_matrix, orot.matrix_to_axis_angle
    tn.scatter_max = lambda src, index, dim_size=None: (o_tn.scatter_max(src, index, dim_size), None)
    tn.scatter_mean = lambda src, index, out=None: o_tn.scatter_mean(src, index, out.shape[-1])

    class Encoder(tn.SMPLXTriplaneEncoder):  # only the two constructors of absent packages are replaced
        def init_smplx_model(self):
            return gen.ToyBody()

        def init_smplx_subdivider(self, subdivide_steps=2):
            self.subdivider_list = []

    enc = Encoder(cfg, sd_mod.SMPLXDecoder(cfg)).eval()
    shapes = {k: list(v.shape) for k, v in enc.state_dict().items()}
    enc.load_state_dict({k: gen.seeded_tensor("smplx_triplane_encoder." + k, v.shape) for k, v in enc.state_dict().items()})
    fine = []
    enc.triplane_downsampler.register_forward_pre_hook(lambda module, args: fine.append(args[0].clone()))
    B, T, S = 2, 1, 16
    gt = smpl_params_gt(gen, B)
    with torch.no_grad():
        img_tokens = gen.rnd(75, B, T, S, cfg.image_feature_dim)
        cam = {"intrinsic": torch.zeros(B, T, 3, 3), "extrinsic": torch.zeros(B, T, 4, 4)}
        planes, _, _ = enc(cam, img_tokens, gt, None)
    assert enc.triplane_resolution == cfg.triplane_resolution and len(fine) == 1
    R = cfg.triplane_resolution
    assert tuple(planes.shape) == (B, T, 3, 64, R, R) and tuple(fine[0].shape) == (B, 3, 64, 3 * R, 3 * R)
    return gen.save("stage1_upsampled", 2, ["src/models/triplane_net.py:66-207,226-244,411-451"],
                    dict(planes=planes, planes_fine=fine[0]),
                    meta=dict(cfg=dict(vars(cfg)), params_encoder=shapes, toy_body=dict(num_verts=40, num_faces=60, seed=5),
                              batch=B, smpl_seed=92, smpl_scale=0.3, smpl_dims=SMPL_DIMS, img_tokens_seed=75,
                              img_tokens_shape=[B, T, S, cfg.image_feature_dim],
                              injected=["smplx.SMPLX := ToyBody (init_smplx_model), pytorch3d subdivider := none",
                                        "torch_scatter.scatter_max / scatter_mean := oracle/triplane_net.py",
                                        "diffusers Attention := OracleAttention",
                                        "pytorch3d rot6d / axis-angle := oracle/rotation.py"]))


def main():
    gen = base_generator()
    if not os.path.isdir(os.path.join(gen.REFERENCE, "src")):
        raise SystemExit(f"{gen.REFERENCE}/src not found: this generator only runs in the build container")
    absent = gen.install_placeholders()
    sys.path.insert(0, gen.REFERENCE)
    sys.dont_write_bytecode = True  # the reference checkout is read-only; leave it untouched
    tr = importlib.import_module("src.models.transformers")
    sd_mod = importlib.import_module("src.models.smplx_decoder")
    tn = importlib.import_module("src.models.triplane_net")
    for m in (tr, sd_mod, tn):
        assert os.path.realpath(m.__file__).startswith(os.path.realpath(gen.REFERENCE)), m.__file__
    gen.PHASE["name"] = "run"
    torch.manual_seed(0)
    torch.set_num_threads(1)  # bit-reproducible sums
    entries = [fixture_downsampler(gen, tn), fixture_upsampled(gen, tn, tr, sd_mod)]
    assert not gen.RUN_EVENTS, f"a placeholder was used while producing fixtures: {gen.RUN_EVENTS}"
    manifest = {"generator": "tests/golden/make_downsampler_golden.py", "base_generator": "tests/golden/make_reference_golden.py",
                "torch": torch.__version__, "absent_packages_mapped_to_inert_placeholders": absent,
                "placeholder_events_during_import": sorted(set(f"{a}: {b}" for a, b in gen.IMPORT_EVENTS)),
                "placeholder_uses_during_run": len(gen.RUN_EVENTS), "fixtures": entries}
    with open(os.path.join(HERE, "ref_downsampler_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    for e in entries:
        print(f"{e['file']:28s} tier {e['tier']}  {e['bytes']:8d} B")
    print("placeholder uses in the run phase:", len(gen.RUN_EVENTS))


if __name__ == "__main__":
    main()
