"""Parity rules of the HIP tile rasterizer against the CPU oracle, shared by the GPU parity suites.

The rules, their tolerances (TOL, FLIP_TOL) and the per-comparison log are report() and compare() of
test_raster_gpu.py, stated in that module's docstring: every unflagged pixel within 1e-3, no more pixels above 1e-3
than the oracle flags, every flagged pixel within one flipped decision (1.2e-2), and the flagged set below 0.5 % of the
image, with geometry decisions (radii, instance counts) exact.  They are re-exported here unchanged.

`compare` holds the last rule per frame.  `compare_small` is its form for frames of fewer than 4096 pixels, where
0.5 % of a frame is a handful of pixels (one pixel of a 16 x 16 frame): there the cap is held over all pixels of the
launch pooled.  The cap exists to keep flags from hiding failures, and pooled it still does; the other three rules are
per pixel and the same in both forms.
"""
import numpy as np

from test_raster_gpu import FLIP_TOL, TOL, compare, report  # noqa: F401  (shared with the other parity suites)

FLAG_CAP = 0.005
SMALL_FRAME = 4096  # pixels: frames below this take compare_small's pooled cap


def compare_small(test, ref, out, frames=None, tol=TOL):
    """`compare` for a launch of frames smaller than SMALL_FRAME pixels, against oracle results the caller already has.

    ref: per-frame dicts of the oracle (color [3,H,W], alpha, unstable; inv_depth, radii and instances where the
    launch is held to them).  out: rasterize()'s result.  frames: the launch frames to compare (default all); ref[i]
    belongs to launch frame frames[i].  Per frame and per pixel the rules are report()'s, unchanged; the flagged-pixel
    cap is held over the pixels of all compared frames together.  Inverse depth and radii are compared where the
    launch produced them, and the instance total when every frame is compared."""
    rgba = out["rgba"].cpu().numpy()
    frames = list(range(rgba.shape[0])) if frames is None else list(frames)
    assert len(frames) == len(ref)
    assert rgba.shape[1] * rgba.shape[2] < SMALL_FRAME, "frames this large take compare()'s per-frame cap"
    flagged = sum(int((r["unstable"] != 0).sum()) for r in ref)
    pixels = sum(int(r["unstable"].size) for r in ref)
    assert flagged < FLAG_CAP * pixels, f"{flagged} of {pixels} pixels of the launch sit on a threshold"
    inv_depth = None if out["inv_depth"] is None else out["inv_depth"].cpu().numpy()
    radii = None if out["radii"] is None else out["radii"].cpu().numpy()
    worst = {}
    for f, r in zip(frames, ref):
        unstable = r["unstable"] != 0
        diffs = [("rgb", np.abs(np.moveaxis(rgba[f, :, :, :3], -1, 0) - r["color"]).max(axis=0)),
                 ("alpha", np.abs(rgba[f, :, :, 3] - r["alpha"]))]
        if inv_depth is not None:
            diffs.append(("inv_depth", np.abs(inv_depth[f] - r["inv_depth"])))
        for name, diff in diffs:
            rec = report(test, f, name, diff, unstable, tol)
            worst[name] = max(worst.get(name, 0.0), rec["max_abs_unflagged"])
        if radii is not None:
            assert np.array_equal(radii[f], r["radii"]), f"frame {f} radii"
    total, over = out["workspace"].status()
    assert not over
    if len(frames) == rgba.shape[0]:
        assert total == sum(r["instances"] for r in ref)
    return worst
