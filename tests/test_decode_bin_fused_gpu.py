"""The triplane decode inside the rasterizer's binning block (amav_rasterize_decode_forward) against the two launches it
replaces (amav_triplane_sample_decode_indexed, then amav_rasterize_forward), in one process and bit for bit: packed
records, frames and the rasterizer's instance counts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F, H, W = 250, 512, 512


@pytest.fixture(scope="module")
def clip():
    """The bench workload (configs[1]): renderer, inputs and the decode inputs of gaussians_from_tokens."""
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd.config import RendererConfig
    from audio_motion_avatar_amd.renderer import Renderer
    from audio_motion_avatar_amd.synthetic import init_random_heads, make_render_inputs

    cfg = RendererConfig(image_size=(H, W), subdivide_steps=0, predict_smplx_params=False, device="cuda")
    r = init_random_heads(Renderer(cfg).eval())
    tokens, smpl, cam = make_render_inputs(F, cfg, seed=42, device="cuda")
    with torch.no_grad():
        w_plane, w_point = r._head_weights()
        tok = tokens[0]
        R = r._plane_resolution(tok)
        flat = {k: v.reshape(F, *v.shape[2:]) for k, v in smpl.items()}
        vertices = r._posed_vertices({k: v.unsqueeze(0) for k, v in flat.items()})
        proj = ops.triplane_project(tok, w_plane, R, region=(ops.points_bbox(vertices), cfg.radius))
        transl = flat["transl"].reshape(F, 3).float()
    return dict(r=r, cfg=cfg, tokens=tokens, smpl=smpl, cam=cam, vertices=vertices, proj=proj, transl=transl,
                w_point=w_point)


def run(c, frames, n=None, hw=(H, W), fuse=True, capacity=None):
    """ops.rasterize(decode=...) of the first `frames` frames and `n` Gaussians -> (packed, rgba, status)."""
    from audio_motion_avatar_amd import ops
    from audio_motion_avatar_amd.renderer import Renderer

    h, w = hw
    idx = c["r"]._gather_idx if n is None else c["r"]._gather_idx[:n].contiguous()
    K = c["cam"]["intrinsic"][0, :frames].float()
    E = c["cam"]["extrinsic"][0, :frames].float()
    view, proj, tanfov, _ = ops.camera_from_intrinsics(K, E, h, w)
    src = ops.decode_source(c["proj"][:frames], c["vertices"][:frames], idx, c["transl"][:frames], c["cfg"].radius,
                            c["w_point"])
    src["out"].fill_(float("nan"))  # every record must be written
    g = Renderer.unpack_gaussians(src["out"])
    ws = None
    if capacity is not None:
        ws = ops.RasterWorkspace(frames, idx.shape[0], h, w, capacity, "cuda")
    out = ops.rasterize(g["xyz"], g["rot"], g["scale"], g["opacity"], g["color"], view, proj, tanfov, h, w,
                        apply_activations=True, clamp_output=True, workspace=ws, decode=src, fuse_decode=fuse)
    status = out["workspace"].status_full()
    assert not status[2]
    return src["out"].clone(), out["rgba"].clone(), status


def same(a, b):
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "packed records differ"
    assert torch.equal(a[1], b[1]), "frames differ"
    assert a[2] == b[2], f"instance counts differ: {a[2]} vs {b[2]}"


@pytest.mark.parametrize("frames", [F, 96, 95])
def test_fused_decode_matches_two_launches(clip, frames):
    """The bench shape, the smallest shard that decodes in the binning block (96 frames) and one frame fewer (two
    launches on both sides)."""
    with torch.no_grad():
        same(run(clip, frames, fuse=True), run(clip, frames, fuse=False))


def test_fused_decode_matches_the_separate_decode_kernel(clip):
    from audio_motion_avatar_amd import ops

    with torch.no_grad():
        packed, _, _ = run(clip, F, fuse=True)
        want = ops.triplane_sample_decode_indexed(clip["proj"], clip["vertices"], clip["r"]._gather_idx, clip["transl"],
                                                  clip["cfg"].radius, clip["w_point"])
    assert torch.equal(packed.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("n", [9999, 4097, 700])
def test_point_counts_off_the_group_size(clip, n):
    with torch.no_grad():
        same(run(clip, 120, n=n, fuse=True), run(clip, 120, n=n, fuse=False))


def test_partial_tiles(clip):
    with torch.no_grad():
        same(run(clip, 100, hw=(500, 472), fuse=True), run(clip, 100, hw=(500, 472), fuse=False))


def test_overflow_retry_reruns_the_fused_launch(clip):
    """An undersized workspace: the first launch overflows, ops.rasterize retries it (decode included) with room."""
    with torch.no_grad():
        fused = run(clip, 100, fuse=True, capacity=100 * 64)
        same(fused, run(clip, 100, fuse=False, capacity=100 * 64))
        same(fused, run(clip, 100, fuse=False))


def test_render_tokens_switch(clip, monkeypatch):
    """Renderer.render_tokens: the argument and AMAV_DECODE_BIN select the path; the results do not depend on it."""
    r, tokens, smpl, cam = (clip[k] for k in ("r", "tokens", "smpl", "cam"))
    with torch.no_grad():
        a = [t.clone() for t in r.render_tokens(tokens[0], smpl, cam, fuse_decode=True)]
        b = [t.clone() for t in r.render_tokens(tokens[0], smpl, cam, fuse_decode=False)]
        monkeypatch.setenv("AMAV_DECODE_BIN", "0")
        c = [t.clone() for t in r.render_tokens(tokens[0], smpl, cam)]
    for x, y in ((a, b), (a, c)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))


def test_fused_render_step_is_hip_graph_capturable(clip):
    """The fused step at 96 frames captured into a HIP graph: replays equal the eager frames, also after an in-place
    input change with an eager pass of the same step between two replays."""
    r, tokens, smpl, cam = (clip[k] for k in ("r", "tokens", "smpl", "cam"))
    Fg = 96
    tok = tokens[0, :Fg].clone()
    sp = {k: v[:, :Fg].clone() for k, v in smpl.items()}
    cm = {k: v[:, :Fg].clone() for k, v in cam.items()}
    ws = [None]
    with torch.no_grad():
        eager, packed_eager = r.render_tokens(tok, sp, cm, workspaces=ws, fuse_decode=True)
        eager, packed_eager = eager.clone(), packed_eager.clone()
        two, _ = r.render_tokens(tok, sp, cm, workspaces=[None], fuse_decode=False)
        assert torch.equal(two, eager)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out, packed = r.render_tokens(tok, sp, cm, workspaces=ws, check_overflow=False, fuse_decode=True)
        torch.cuda.current_stream().wait_stream(side)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(packed, packed_eager), "replay differs from the eager pass"
        assert not ws[0].status()[1]
        sp["global_orient"].add_(0.3)
        want, _ = r.render_tokens(tok, sp, cm, workspaces=[None], fuse_decode=True)
        want = want.clone()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and not torch.equal(want, eager), "replay did not follow the in-place change"
