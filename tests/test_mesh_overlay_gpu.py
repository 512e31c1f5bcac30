"""The mesh overlay kernels (csrc/mesh.hip through ops.mesh_overlay) against the numpy model (mesh_model.py) on the
scenes of mesh_scenes.py, then the module (mesh_overlay.py) and the demo's --smplx-out."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_model as mm
import mesh_scenes
from mesh_scenes import ZNEAR

pytestmark = pytest.mark.gpu

NEAR_TIE_CAP = 0.01
BACKGROUND = (0.25, 0.5, 0.75)
K_SHADE = mm.shade_k()


def frames_for(name, channels):
    s = mesh_scenes.SCENES[name]()
    g = torch.Generator().manual_seed(5)
    return torch.rand(s["vertices"].shape[0], s["H"], s["W"], channels, generator=g)


@functools.lru_cache(maxsize=None)
def kernel(name, cull=True, small_box=None, channels=3, only_frame=None, long_faces=False):
    """ops.mesh_overlay on a scene with every optional output -> dict of numpy arrays (computed once per variant)."""
    from audio_motion_avatar_amd import ops

    s = mesh_scenes.SCENES[name]()
    pick = slice(None) if only_frame is None else slice(only_frame, only_frame + 1)
    dev = lambda a, dtype=torch.float32: torch.as_tensor(a[pick]).to("cuda", dtype)
    faces = torch.as_tensor(s["faces"]).cuda()
    frames = frames_for(name, channels)[pick].cuda() if channels else None
    out = ops.mesh_overlay(dev(s["vertices"]), faces.long() if long_faces else faces, dev(s["K"]), dev(s["E"]), s["H"],
                           s["W"], frames=frames, transl=None if s["transl"] is None else dev(s["transl"]), znear=ZNEAR,
                           cull_backfaces=cull, background=BACKGROUND, want_depth=True, want_face_index=True,
                           want_screen=True, want_shade=True, small_box=small_box)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def model_on_kernel_screen(name, cull=True):
    """The model run on the kernel's own snapped coordinates, with depths from its fp64 projection."""
    s = mesh_scenes.SCENES[name]()
    got = kernel(name, cull)
    return [mm.render(s["vertices"][f], s["faces"], s["K"][f], s["E"][f], s["H"], s["W"],
                      None if s["transl"] is None else s["transl"][f], screen=got["screen"][f], znear=ZNEAR,
                      cull_backfaces=cull) for f in range(s["vertices"].shape[0])]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


SCENE_NAMES = sorted(mesh_scenes.SCENES)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_projection_lands_within_one_snapped_unit(name):
    """fp32 projection errs by about 1e-4 px here, far below the 1/256 px cell: it can move a vertex across one rounding
    boundary at most."""
    got = kernel(name)
    for f, ref in enumerate(mesh_scenes.model_frames(name)):
        front = ref["p_cam"][:, 2] >= ZNEAR
        err = np.abs(got["screen"][f].astype(np.int64) - ref["screen"])[front]
        print(f"{name}[{f}]: {front.sum()} vertices, max snapped error {err.max()} units, moved {(err > 0).mean():.4f}")
        assert err.max() <= 1


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_coverage_is_exact_and_depth_matches(name):
    """face_index equals the model's at EVERY pixel that is not a near-tie, -1 included; inside the mask the depth is
    within 1e-5 relative of the model's fp64 depth, outside it is exactly 0."""
    got = kernel(name)
    for f, ref in enumerate(model_on_kernel_screen(name)):
        covered = ref["face_index"] >= 0
        share = ref["near_tie"].sum() / max(1, covered.sum())
        compare = ~ref["near_tie"]
        wrong = (got["face_index"][f] != ref["face_index"]) & compare
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(covered & compare, np.abs(got["depth"][f] - ref["depth"]) / ref["depth"], 0.0)
        print(f"{name}[{f}]: covered {covered.sum()}, near-tie share {share:.4f}, wrong {wrong.sum()}, "
              f"max relative depth error {rel.max():.2e}, status {got['status'][f].tolist()}")
        assert share <= NEAR_TIE_CAP
        assert not wrong.any()
        assert np.array_equal(got["face_index"][f] >= 0, covered)  # a near-tie changes the winner, never the mask
        assert rel.max() <= 1e-5
        assert (got["depth"][f][~covered] == 0).all() and (got["depth"][f][covered] > 0).all()
        assert tuple(got["status"][f].tolist()) == ref["status"]


def test_sphere_is_watertight_and_pins_the_winding():
    """A convex closed mesh: every row and column of the covered set is one run (no hole), every winner is a front face,
    and the depth at the centre is the NEAR side of the sphere (2.0 m, not 3.0 m): front = negative doubled area."""
    s = mesh_scenes.sphere()
    got, ref = kernel("sphere"), model_on_kernel_screen("sphere")[0]
    mask = got["face_index"][0] >= 0
    assert 400 < mask.sum() < 600
    for line in list(mask) + list(mask.T):
        on = np.nonzero(line)[0]
        assert on.size == 0 or on.size == on[-1] - on[0] + 1
    assert ref["front"][got["face_index"][0][mask]].all()
    r, c = int(s["K"][0, 1, 2]), int(s["K"][0, 0, 2])  # the pixel under the sphere's centre
    assert 2.0 <= got["depth"][0, r, c] < 2.01
    assert (got["rgb"][0, r - 2:r + 3, c - 2:c + 3] > 0.9).all()  # k = 1.22 saturates a face that looks at the camera
    both = kernel("sphere", cull=False)
    assert np.array_equal(both["face_index"][0] >= 0, mask)
    assert (both["rgb"][0, r - 2:r + 3, c - 2:c + 3] > 0).all()
    # with culling off a back face keeps the shade its reversed twin would have: nothing is lit from behind
    kept_back = ~ref["front"] & model_on_kernel_screen("sphere", cull=False)[0]["kept"]
    assert kept_back.sum() > 300 and (got["shade"][0][kept_back] == 0).all()
    # (all of them but the band between the silhouette and the plane through the centre, whose reversed normals still
    # point away from the light; test_shade_matches_fp64 compares the values)
    assert (both["shade"][0][kept_back].max(axis=1) > 0).mean() > 0.5


@pytest.mark.parametrize("name", ["quad", "body"])
def test_both_tiers_agree_bit_for_bit(name):
    """small_box = 0 sends every face through the wave-per-face tier; at the default the quad's two faces take it and
    everything else the thread-per-face loop."""
    small, large = kernel(name), kernel(name, small_box=0)
    for key in ("face_index", "depth", "rgb", "shade", "status"):
        assert same_bits(small[key], large[key]), key
    if name == "quad":
        assert same_bits(kernel(name, small_box=1 << 30)["face_index"], small["face_index"])  # and none takes it


def test_dropped_faces_are_counted_and_leave_the_image_alone():
    c, d = kernel("quad"), kernel("quad_with_drops")
    assert d["status"].tolist() == [[1, 1]] and c["status"].tolist() == [[0, 0]]
    for key in ("face_index", "depth", "rgb"):
        assert same_bits(c[key], d[key]), key
    assert (d["shade"][0, 3:] == 0).all()
    assert set(np.unique(c["face_index"])) == {0, 1, 2}


@pytest.mark.parametrize("name,cull", [(n, True) for n in SCENE_NAMES] + [("sphere", False)])
def test_shade_matches_fp64(name, cull):
    """Per face: |shade - fp64| <= k * 16 * 2^-24 * max|p_cam| / min edge length + 1e-6.  The normal is a cross product of
    edge DIFFERENCES of camera-space points: each difference carries the rounding of its operands, about 2^-24 max|p_cam|,
    against an edge length that can be far smaller (cancellation); 16 covers the handful of such terms."""
    s = mesh_scenes.SCENES[name]()
    got = kernel(name, cull)
    for f, ref in enumerate(model_on_kernel_screen(name, cull)):
        kept = ref["kept"]
        want = mm.shade(ref["p_cam"], s["faces"], K_SHADE, ref["front"])
        p = ref["p_cam"][s["faces"][kept].astype(np.int64)]
        edges = np.linalg.norm(p - np.roll(p, 1, axis=1), axis=2).min(axis=1)
        bound = K_SHADE.max() * 16 * 2.0 ** -24 * np.abs(p).max(axis=(1, 2)) / edges + 1e-6
        err = np.abs(got["shade"][f][kept] - want[kept]).max(axis=1)
        print(f"{name}[{f}]: {kept.sum()} faces, max shade error {err.max():.2e}, max error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
        assert (got["shade"][f][~kept] == 0).all()


@pytest.mark.parametrize("channels", [3, 4, 0])
@pytest.mark.parametrize("name", ["body", "quad_with_drops", "sphere"])
def test_composite_is_bitwise(name, channels):
    """Outside the mask the input frame (3 or 4 channels) or the background colour, inside shade[face_index], bit for bit."""
    got = kernel(name, channels=channels)
    mask = got["face_index"] >= 0
    assert same_bits(got["face_index"], kernel(name)["face_index"])
    if channels:
        under = frames_for(name, channels).numpy()[..., :3]
    else:
        under = np.broadcast_to(np.array(BACKGROUND, np.float32), got["rgb"].shape)
    assert same_bits(got["rgb"][~mask], np.ascontiguousarray(under[~mask]))
    for f in range(mask.shape[0]):
        assert same_bits(got["rgb"][f][mask[f]], got["shade"][f][got["face_index"][f][mask[f]]])
    assert mask.any() and (name == "quad_with_drops" or (~mask).any())


def test_runs_are_reproducible_and_frames_independent():
    from audio_motion_avatar_amd import ops

    a = kernel("body")
    kernel.cache_clear()
    b = kernel("body")
    for key in a:
        assert same_bits(a[key], b[key]), key
    for f in range(3):
        alone = kernel("body", only_frame=f)
        for key in a:
            assert same_bits(alone[key][0], a[key][f]), (key, f)
    assert same_bits(kernel("sphere", long_faces=True)["face_index"], kernel("sphere")["face_index"])  # int64 faces: converted
    # a caller's workspace is used as it is, and one byte less is refused
    s = mesh_scenes.sphere()
    args = [torch.as_tensor(s[k]).cuda() for k in ("vertices", "faces", "K", "E")] + [s["H"], s["W"]]
    need = ops._lib.lib().amav_mesh_overlay_workspace_bytes(1, s["vertices"].shape[1], s["faces"].shape[0], s["H"], s["W"])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    again = ops.mesh_overlay(*args, znear=ZNEAR, background=BACKGROUND, want_face_index=True, workspace=ws)
    assert same_bits(again["face_index"].cpu().numpy(), kernel("sphere", channels=0)["face_index"])
    with pytest.raises(ops.AmavError, match="workspace"):
        ops.mesh_overlay(*args, workspace=ws[:-1])


def test_draw_smplx_on_image_stacks_frame_over_overlay():
    """[B,T,3,H,W] -> [B*T, 2H, W, 3]: the top half is the input bit for bit, the bottom half differs from it only where
    a face won; BodyModel poses the batch on the device and transl reaches the kernel."""
    from audio_motion_avatar_amd.body_model import BodyModel
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.mesh_overlay import SimpleMeshRenderer, draw_smplx_on_image
    from audio_motion_avatar_amd.synthetic import make_render_inputs

    B, T, H, W = 2, 2, 50, 70
    _, smpl, cam = make_render_inputs(T, RendererConfig(image_size=(H, W), device="cuda"), seed=3, device="cuda", batch=B)
    body = BodyModel.synthetic_model(seed=42, device="cuda")
    renderer = SimpleMeshRenderer(body.faces, H, W)
    images = torch.rand(B, T, 3, H, W, generator=torch.Generator().manual_seed(9)).cuda()
    out, face_index = draw_smplx_on_image(images, smpl, cam["intrinsic"], cam["extrinsic"], body, renderer,
                                          return_face_index=True)
    assert out.shape == (B * T, 2 * H, W, 3) and out.dtype == torch.float32 and out.is_cuda
    frames = images.reshape(B * T, 3, H, W).permute(0, 2, 3, 1)
    assert torch.equal(out[:, :H], frames)
    changed = (out[:, H:] != frames).any(dim=-1)
    won = face_index >= 0
    assert not (changed & ~won).any() and 0.05 < won.float().mean() < 0.9 and changed.sum() > 0.9 * won.sum()
    assert torch.equal(draw_smplx_on_image(images, smpl, cam["intrinsic"], cam["extrinsic"], body, renderer), out)
    # without transl the body sits on the camera: a different picture, so transl did reach the kernel
    one = renderer.render_mesh(body(**{k: v.reshape(B * T, -1) for k, v in smpl.items()}).vertices[0], frames[0],
                               cam["intrinsic"][0, 0], cam["extrinsic"][0, 0])
    assert one.shape == (H, W, 3) and not torch.equal(one, out[0, H:])


def test_demo_writes_the_stacked_clip(tmp_path, monkeypatch):
    """--smplx-out: 7 frames of 128 x 48, the top half of each the frame of --out byte for byte, the bottom half with the
    mesh over it.  Without the flag the demo takes the path it took before: rollout() is called without return_smplx and
    returns the dict it always returned, the overlay is never reached, and no further file appears."""
    import wave

    from audio_motion_avatar_amd import demo, harness, mesh_overlay

    g = torch.Generator().manual_seed(1)
    pcm = (torch.randn(1, 22050, generator=g) * 0.1 * 32768).clamp(-32768, 32767).short()
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(22050)
        w.writeframes(pcm.numpy().tobytes())
    common = ["--frames", "7", "--image-size", "64", "48", "--audio", str(tmp_path / "a.wav")]
    a, b, plain = tmp_path / "clip.rgb", tmp_path / "mesh.rgb", tmp_path / "plain.rgb"
    assert demo.main(common + ["--out", str(a), "--smplx-out", str(b)]) == 0
    assert os.path.getsize(b) == 7 * 128 * 48 * 3
    meta = json.load(open(str(b) + ".json"))
    assert (meta["height"], meta["width"], meta["frames"]) == (128, 48, 7)
    top = np.fromfile(a, dtype=np.uint8).reshape(7, 64, 48, 3)
    stacked = np.fromfile(b, dtype=np.uint8).reshape(7, 128, 48, 3)
    assert np.array_equal(stacked[:, :64], top)
    assert (stacked[:, 64:] != top).any()

    calls = []
    rollout = harness.AudioDrivenAvatar.rollout

    def spy(self, *args, **kwargs):
        out = rollout(self, *args, **kwargs)
        calls.append((kwargs, sorted(out)))
        return out

    def unreachable(*args, **kwargs):
        raise AssertionError("the overlay ran without --smplx-out")

    monkeypatch.setattr(harness.AudioDrivenAvatar, "rollout", spy)
    monkeypatch.setattr(mesh_overlay, "draw_smplx_on_image", unreachable)
    assert demo.main(common + ["--out", str(plain)]) == 0
    assert calls == [({"return_smplx": False}, ["images", "smplx_tokens", "triplanes"])]
    assert os.path.getsize(plain) == 7 * 64 * 48 * 3 and json.load(open(str(plain) + ".json"))["height"] == 64
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.wav", "clip.rgb", "clip.rgb.json", "mesh.rgb", "mesh.rgb.json",
                                                          "plain.rgb", "plain.rgb.json"]


def test_demo_interleaved_mesh_clip(tmp_path):
    """--interleave --smplx-out: rollout_interleaved hands back the SMPL-X parameters zipped like the frames."""
    from audio_motion_avatar_amd import demo

    a, b = tmp_path / "clip.rgb", tmp_path / "mesh.rgb"
    assert demo.main(["--frames", "12", "--image-size", "64", "48", "--interleave", "--out", str(a), "--smplx-out", str(b)]) == 0
    top = np.fromfile(a, dtype=np.uint8).reshape(12, 64, 48, 3)
    stacked = np.fromfile(b, dtype=np.uint8).reshape(12, 128, 48, 3)
    assert np.array_equal(stacked[:, :64], top)
    assert all((stacked[i, 64:] != top[i]).any() for i in range(12))
