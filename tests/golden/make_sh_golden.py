#!/usr/bin/env python3
"""Golden vectors for the spherical-harmonic colour branch, produced by RUNNING THE REFERENCE'S OWN eval_sh
(src/utils/graphic_utils.py:707-762) on the CPU of the build container, in fp32, inside the statements that surround it
in render_one (src/models/renderer.py:541-545): the coefficients reshaped to [N,K,3] and transposed, the direction
(p - campos) / |p - campos|, eval_sh, clamp_min(. + 0.5, 0).  tests/golden/make_reference_golden.py is imported as a
module for its placeholder machinery (absent third-party packages become inert placeholders; any use of one while
fixture data is produced raises) and its run-phase "zero placeholder uses" assertion.

Cases (tests/sh_model.py builds the inputs from seeds): degrees 0..4 with (degree+1)^2 stored coefficients, and degree 1
with 16 stored coefficients; N = 257 Gaussians shared by 3 cameras, coefficients ~ N(0, 0.5^2), every |p - campos| >= 0.5.
Per case the fixture holds means3d [1,N,3], sh [1,N,K,3], campos [3,3], degree and the reference's colours [3,N,3].
Only data travels, none of the reference's text.

Run:  python tests/golden/make_sh_golden.py      (needs the reference checkout; CPU only)
"""
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CASES = [("deg0", 0, None), ("deg1", 1, None), ("deg2", 2, None), ("deg3", 3, None), ("deg4", 4, None), ("deg1_k16", 1, 16)]
N, CAMERAS, SEED = 257, 3, 8800


def base_generator():
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(HERE, "make_reference_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # defines functions only
    return mod


def reference_colours(gu, degree, points, coeffs, centre):
    """What renderer.py:541-545 computes for one camera, around the reference's own eval_sh: points [N,3], coeffs
    [N,3*K], centre [3] -> colours [N,3]."""
    n = points.shape[0]
    per_channel = coeffs.reshape(n, -1, 3).transpose(1, 2)           # [N,3,K]: eval_sh wants the coefficients last
    offset = points - centre.repeat(n, 1)
    unit = offset / offset.norm(dim=1, keepdim=True)
    return torch.clamp_min(gu.eval_sh(degree, per_channel, unit) + 0.5, 0.0)


def main():
    gen = base_generator()
    if not os.path.isdir(os.path.join(gen.REFERENCE, "src")):
        raise SystemExit(f"{gen.REFERENCE}/src not found: this generator only runs in the build container")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sh_model

    absent = gen.install_placeholders()
    sys.path.insert(0, gen.REFERENCE)
    sys.dont_write_bytecode = True  # the reference checkout is read-only; leave it untouched
    gu = importlib.import_module("src.utils.graphic_utils")
    assert os.path.realpath(gu.__file__).startswith(os.path.realpath(gen.REFERENCE)), gu.__file__
    gen.PHASE["name"] = "run"
    torch.set_num_threads(1)
    arrays, meta = {}, {}
    for i, (name, degree, stored) in enumerate(CASES):
        c = sh_model.case(SEED + i, degree, CAMERAS, N, K=stored, shared=True)
        xyzs, colors = c["means3d"][0], c["sh"][0].reshape(N, -1)
        assert xyzs.dtype == colors.dtype == c["campos"].dtype == torch.float32
        out = torch.stack([reference_colours(gu, degree, xyzs, colors, c["campos"][f]) for f in range(CAMERAS)])
        assert out.shape == (CAMERAS, N, 3) and out.dtype == torch.float32
        dist = (xyzs[None] - c["campos"][:, None]).norm(dim=-1).min().item()
        assert dist >= 0.5, dist
        clamped = (out == 0).float().mean().item()
        arrays.update({f"{name}/means3d": c["means3d"], f"{name}/sh": c["sh"], f"{name}/campos": c["campos"],
                       f"{name}/degree": np.asarray(degree), f"{name}/colors": out})
        meta[name] = dict(degree=degree, coefficients=int(c["K"]), clamped_share=round(clamped, 4),
                          nearest_camera=round(dist, 3))
        print(f"{name:9s} degree {degree} K {c['K']:2d} clamped {clamped:.3f} nearest camera {dist:.2f}")
    assert not gen.RUN_EVENTS, f"a placeholder was used while producing fixtures: {gen.RUN_EVENTS}"
    entry = gen.save("sh", 1, ["src/utils/graphic_utils.py:707-762", "src/models/renderer.py:541-545"], arrays,
                     meta=dict(cases=meta, gaussians=N, cameras=CAMERAS, seed=SEED))
    assert entry["bytes"] < 400000, entry["bytes"]
    manifest = {"generator": "tests/golden/make_sh_golden.py", "base_generator": "tests/golden/make_reference_golden.py",
                "torch": torch.__version__, "absent_packages_mapped_to_inert_placeholders": absent,
                "placeholder_events_during_import": sorted(set(f"{a}: {b}" for a, b in gen.IMPORT_EVENTS)),
                "placeholder_uses_during_run": len(gen.RUN_EVENTS), "fixtures": [entry]}
    with open(os.path.join(HERE, "ref_sh_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    print(f"{entry['file']:28s} tier {entry['tier']}  {entry['bytes']:8d} B")
    print("placeholder uses in the run phase:", len(gen.RUN_EVENTS))


if __name__ == "__main__":
    main()
