"""The demo's second clip: the predicted SMPL-X mesh drawn over the rendered frames (src/main2.py:213-220,296-303).

`SimpleMeshRenderer` and `draw_smplx_on_image` keep the names and signatures of src/utils/graphic_utils.py:782-944, so

    from src.utils.graphic_utils import SimpleMeshRenderer, draw_smplx_on_image

becomes `from audio_motion_avatar_amd.mesh_overlay import ...`.  The reference builds one pyrender scene and one trimesh
per frame on an offscreen GL context and brings every frame through the host; here the whole batch is ONE call of
ops.mesh_overlay (csrc/mesh.hip: a z-buffered triangle rasterizer, flat shading, composite) and nothing leaves the
device.  Shading restates pyrender's metallic-roughness material at metallic 0 / roughness 1 under the reference's
directional light of intensity 5 at the camera: the diffuse term 0.96 * base_color * intensity / pi * max(0, n . l).  Its
specular lobe (about 0.02 at roughness 1) is left out, and other material values are refused.  pyrender is not in the
image, so parity with it is unpinned.

One deliberate difference: the reference's demo hands float frames in [0, 1] to code written for uint8 images
(`out = img * (1 - mask) + color * mask; return out / 255`), so its pixels outside the mesh come out as img / 255, which
is black to the eye.  Here the frame is kept under the mask, which is what render_mesh's docstring describes.
"""
import numpy as np
import torch

from . import ops

LIGHT_INTENSITY = 5.0  # graphic_utils.py:850


def _check_material(metallic, roughness, emissive):
    if metallic != 0.0 or roughness != 1.0 or emissive is not None:
        raise NotImplementedError("mesh overlay: only the reference's material (metallic=0.0, roughness=1.0, no emissive "
                                  "term) is implemented: the shade is the diffuse term alone")


class SimpleMeshRenderer:
    """graphic_utils.py:782-860 without the GL context: holds the faces (as an int32 device tensor, per device) and the
    image size."""

    def __init__(self, faces, H: int, W: int):
        self.faces = faces
        self.width, self.height = int(W), int(H)
        self._device_faces = {}

    def faces_on(self, device):
        device = torch.device(device)
        if device not in self._device_faces:
            faces = self.faces if isinstance(self.faces, torch.Tensor) else torch.as_tensor(np.asarray(self.faces, dtype=np.int64))
            self._device_faces[device] = faces.to(device=device, dtype=torch.int32).contiguous()
        return self._device_faces[device]

    def render_batch(self, vertices, images, K, E, transl=None, base_color=(0.8, 0.8, 0.8), **outputs):
        """vertices [F,V,3], images fp32 [F,H,W,3|4] in [0,1] on the device, K [F,3,3], E [F,4,4] -> ops.mesh_overlay's
        dict (rgb [F,H,W,3]); `outputs`: its want_* flags."""
        return ops.mesh_overlay(vertices, self.faces_on(vertices.device), K, E, self.height, self.width, frames=images,
                                transl=transl, base_color=base_color, light_intensity=LIGHT_INTENSITY, **outputs)

    def render_mesh(self, vertices, image, K, E, base_color=(0.8, 0.8, 0.8), metallic=0.0, roughness=1.0, emissive=None):
        """One mesh over one image: vertices (V,3), image (H,W,3) fp32 in [0,1] on the device, K (3,3), E (4,4)
        world-to-camera -> (H,W,3) fp32 on the device: the shaded mesh where it covers a pixel, the image elsewhere."""
        _check_material(metallic, roughness, emissive)
        return self.render_batch(vertices[None], image[None], K[None], E[None], base_color=base_color)["rgb"][0]


@torch.no_grad()
def draw_smplx_on_image(images, smplx_params, Ks, Es, smplx_model, renderer, return_face_index=False):
    """graphic_utils.py:892-944.  images [B,T,3,H,W] fp32 in [0,1], smplx_params: dict of [B,T,dim] tensors (the
    renderer's `pred_smplx_future`), Ks [B,T,3,3], Es [B,T,4,4], smplx_model: a BodyModel -> [B*T, 2H, W, 3] fp32 on the
    device: the input frame on top, the frame with the mesh drawn over it below.  `transl` goes to the kernel
    (BodyModel.forward takes none).  return_face_index: also the int32 [B*T,H,W] face ids of the overlay, -1 off the mesh."""
    B, T, _, H, W = images.shape
    n = B * T
    frames = images.reshape(n, 3, H, W).permute(0, 2, 3, 1).float().contiguous()
    r = lambda k: smplx_params[k].reshape(n, -1).to(frames.device).float()
    vertices = smplx_model(global_orient=r("global_orient"), body_pose=r("body_pose"), betas=r("betas"),
                           left_hand_pose=r("left_hand_pose"), right_hand_pose=r("right_hand_pose"),
                           jaw_pose=r("jaw_pose"), leye_pose=r("leye_pose"), reye_pose=r("reye_pose"),
                           expression=r("expression")).vertices
    transl = r("transl") if smplx_params.get("transl") is not None else None
    out = renderer.render_batch(vertices, frames, Ks.reshape(n, 3, 3).float(), Es.reshape(n, 4, 4).float(), transl=transl,
                                want_face_index=return_face_index)
    stacked = torch.cat([frames, out["rgb"]], dim=1)
    return (stacked, out["face_index"]) if return_face_index else stacked
