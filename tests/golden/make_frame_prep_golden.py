#!/usr/bin/env python3
"""Golden vectors for the training-clip frame preparation, produced by RUNNING THE REFERENCE'S OWN DATASET CODE on the
CPU of the build container: GaussianAudioDataset.__getitem__ (src/datasets/dataset_speech_vid.py:147-293, pad_image
:319-331) on the cases of tests/frame_prep_cases.py.  tests/golden/make_reference_golden.py is imported as a module for
its placeholder machinery (absent third-party packages, torchaudio among them, become inert placeholders; any use of one
while fixture data is produced raises) and its run-phase "zero placeholder uses" assertion.

The dataset object is made with object.__new__ (its constructor extracts audio features with wav2vec2) and given the
attributes __getitem__ reads.  Each case's frames and masks are written as PNG with Pillow into a temporary directory,
beside one JSON parameter file per frame; `d_no_mask` has no mask file.  The reference hard-codes a 1024 x 1024 crop
(12.6 MB per frame), so the fixture keeps

  <case>/images    whole, for the 96 x 72 cases
  <case>/cropped   fp32 [F,3,P]: `cropped_images` at the P positions of frame_prep_cases.golden_positions() (rows and
                   columns 0, 1, 511, 512, 1022, 1023 in full and every 41st pixel of the rest), row-major

Nothing of the reference travels: the fixtures hold outputs only, the inputs are formulas.  Interpolated fp32 values
hardly compress (about a byte per value stays noise), so the cases are split over two files to keep each well below
the repository's limit for a committed file: ref_frame_prep.npz (a-e) and ref_frame_prep_more.npz (f-h), one manifest.

Run:  python tests/golden/make_frame_prep_golden.py      (needs the reference checkout and Pillow; CPU only)
"""
import importlib
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def base_generator():
    spec = importlib.util.spec_from_file_location("make_reference_golden", os.path.join(HERE, "make_reference_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # defines functions only
    return mod


def write_case(root, case):
    from PIL import Image

    os.makedirs(os.path.join(root, "imgs_png"))
    os.makedirs(os.path.join(root, "samurai_seg"))
    os.makedirs(os.path.join(root, "smplx_params"))
    files = []
    for f in range(case["frames"].shape[0]):
        path = os.path.join(root, "imgs_png", f"{f:05d}.png")
        Image.fromarray(case["frames"][f], "RGB").save(path)
        if case["masks"] is not None:
            Image.fromarray(case["masks"][f], "L").save(os.path.join(root, "samurai_seg", f"{f:05d}.png"))
        params = dict(betas=[0.0] * 10, trans=[0.0] * 3, root_pose=[0.0] * 3, body_pose=[0.0] * 63, lhand_pose=[0.0] * 45,
                      rhand_pose=[0.0] * 45, jaw_pose=[0.0] * 3, leye_pose=[0.0] * 3, reye_pose=[0.0] * 3,
                      pad_ratio=case["pad_ratio"], focal=[500.0, 500.0], princpt=[case["W"] / 2, case["H"] / 2])
        with open(os.path.join(root, "smplx_params", f"{f:05d}.json"), "w") as fh:
            json.dump(params, fh)
        files += [path, path]  # __getitem__ steps through image_files by two
    return files


def run_case(ds_mod, case):
    with tempfile.TemporaryDirectory() as root:
        files = write_case(root, case)
        ds = object.__new__(ds_mod.GaussianAudioDataset)
        ds.root_dir, ds.image_dir, ds.smplx_params_dir = root, os.path.join(root, "imgs_png"), os.path.join(root, "smplx_params")
        ds.image_files, ds.clip_length = files, len(files) // 2
        ds.audio_features = [np.zeros(4, np.float32)] * len(files)
        item = ds[0]
    return item["images"].numpy(), item["cropped_images"].numpy()


def main():
    gen = base_generator()
    if not os.path.isdir(os.path.join(gen.REFERENCE, "src")):
        raise SystemExit(f"{gen.REFERENCE}/src not found: this generator only runs in the build container")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import frame_prep_cases as fc

    absent = gen.install_placeholders()
    try:  # installed, but its wav2vec2 classes may not import (they pull in torchvision): then it counts as absent
        from transformers import Wav2Vec2Model, Wav2Vec2Processor  # noqa: F401
    except Exception:
        for key in [k for k in sys.modules if k.split(".")[0] == "transformers"]:
            del sys.modules[key]
        sys.modules["transformers"] = gen._PlaceholderModule("transformers")
        absent = sorted(absent + ["transformers"])
    sys.path.insert(0, gen.REFERENCE)
    sys.dont_write_bytecode = True  # the reference checkout is read-only; leave it untouched
    ds_mod = importlib.import_module("src.datasets.dataset_speech_vid")
    assert os.path.realpath(ds_mod.__file__).startswith(os.path.realpath(gen.REFERENCE)), ds_mod.__file__
    gen.PHASE["name"] = "run"
    torch.set_num_threads(1)
    keep = fc.golden_positions()
    shapes = {}
    files = {"frame_prep": ({}, fc.CASES[:5]), "frame_prep_more": ({}, fc.CASES[5:])}
    for name in fc.CASES:
        arrays = files["frame_prep" if name in fc.CASES[:5] else "frame_prep_more"][0]
        case = fc.case(name)
        images, cropped = run_case(ds_mod, case)
        assert cropped.shape[1:] == (3, fc.REF_SIDE, fc.REF_SIDE) and cropped.dtype == np.float32
        arrays[name + "/cropped"] = cropped[:, :, keep]
        if name in fc.SMALL_IMAGES:
            arrays[name + "/images"] = images
        shapes[name] = dict(images=list(images.shape), frames=int(cropped.shape[0]))
    assert not gen.RUN_EVENTS, f"a placeholder was used while producing fixtures: {gen.RUN_EVENTS}"
    entries = [gen.save(stem, 1, ["src/datasets/dataset_speech_vid.py:147-293,319-331"], part,
                        meta=dict(cases={n: shapes[n] for n in names}, positions=int(keep.sum()), edge=list(fc.EDGE),
                                  stride=fc.STRIDE)) for stem, (part, names) in files.items()]
    assert all(e["bytes"] < 1000000 for e in entries), [e["bytes"] for e in entries]
    manifest = {"generator": "tests/golden/make_frame_prep_golden.py", "base_generator": "tests/golden/make_reference_golden.py",
                "torch": torch.__version__, "absent_packages_mapped_to_inert_placeholders": absent,
                "placeholder_events_during_import": sorted(set(f"{a}: {b}" for a, b in gen.IMPORT_EVENTS)),
                "placeholder_uses_during_run": len(gen.RUN_EVENTS), "fixtures": entries}
    with open(os.path.join(HERE, "ref_frame_prep_manifest.json"), "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
    for e in entries:
        print(f"{e['file']:28s} tier {e['tier']}  {e['bytes']:8d} B")
    print("placeholder uses in the run phase:", len(gen.RUN_EVENTS))


if __name__ == "__main__":
    main()
