"""Host side of the data-parallel step (amav_grads_pack / amav_tensors_fingerprint): the bucket layout, the refusals that
come back before the device is touched, the calls that have nothing to do, and the Python names."""
import inspect

import pytest

from abi_support import ERR_INVALID, FAKE, lib  # noqa: F401 (lib: fixture)


def _pack(lib, **over):
    a = dict(tensors=FAKE, T=3, chunks=FAKE, C=5, chunk=64, offsets=FAKE, bucket=FAKE, numel=1024, scale=0.5, zero=0)
    a.update(over)
    return lib.amav_grads_pack(a["tensors"], a["T"], a["chunks"], a["C"], a["chunk"], a["offsets"], a["bucket"], a["numel"],
                               a["scale"], a["zero"], None)


def _fingerprint(lib, **over):
    a = dict(tensors=FAKE, T=3, chunks=FAKE, C=5, chunk=64, which=0, partial=FAKE, out=FAKE)
    a.update(over)
    return lib.amav_tensors_fingerprint(a["tensors"], a["T"], a["chunks"], a["C"], a["chunk"], a["which"], a["partial"],
                                        a["out"], None)


def _refused(lib, rc, *texts):
    message = lib.amav_last_error()
    return rc == ERR_INVALID and all(t in message for t in texts)


def test_bucket_offsets_known_answers():
    from audio_motion_avatar_amd import ops

    numels = [1, 3, 64, 65, 0, 12293]
    assert ops.bucket_offsets(numels) == ([0, 64, 128, 192, 320, 320], 12672)
    assert ops.bucket_offsets(numels, align=64) == ops.bucket_offsets(numels)
    # align 4: 1 -> 4, 3 -> 8, 64 -> 72, 65 -> 137 -> 140, the empty tensor stays at 140, 140 + 12293 = 12433 -> 12436
    assert ops.bucket_offsets(numels, align=4) == ([0, 4, 8, 72, 140, 140], 12436)
    assert ops.bucket_offsets([], align=64) == ([], 0)
    assert ops.bucket_offsets([0, 0]) == ([0, 0], 0)
    assert ops.bucket_offsets([128, 64]) == ([0, 128], 192)                  # exact multiples leave no gap
    offsets, total = ops.bucket_offsets([5, 70000, 17], align=64)
    assert all(o % 64 == 0 for o in offsets) and total % 64 == 0 and total >= offsets[-1] + 17
    for bad in (lambda: ops.bucket_offsets([4, -1]), lambda: ops.bucket_offsets([4], align=3),
                lambda: ops.bucket_offsets([4], align=0), lambda: ops.bucket_offsets([4], align=-64)):
        with pytest.raises(ValueError, match="bucket_offsets"):
            bad()


def test_pack_refusals(lib):
    name = b"amav_grads_pack"
    for arg in ("tensors", "chunks"):
        assert _refused(lib, _pack(lib, **{arg: None}), name, b"NULL table"), arg
    for arg in ("T", "C"):
        assert _refused(lib, _pack(lib, **{arg: -1}), name, b"negative"), arg
    for chunk in (0, -4):
        assert _refused(lib, _pack(lib, chunk=chunk), name, b"chunk"), chunk
    for arg in ("offsets", "bucket"):
        assert _refused(lib, _pack(lib, **{arg: None}), name, b"NULL pointer"), arg
    assert _refused(lib, _pack(lib, numel=-1), name, b"bucket_numel")
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert _refused(lib, _pack(lib, scale=scale), name, b"scale"), scale
    assert _refused(lib, _pack(lib, T=0, chunk=0), name, b"chunk")           # an empty problem still has its sizes checked
    assert _refused(lib, _pack(lib, C=0, scale=float("nan")), name, b"scale")


def test_fingerprint_refusals(lib):
    name = b"amav_tensors_fingerprint"
    for arg in ("tensors", "chunks"):
        assert _refused(lib, _fingerprint(lib, **{arg: None}), name, b"NULL table"), arg
    for arg in ("T", "C"):
        assert _refused(lib, _fingerprint(lib, **{arg: -1}), name, b"negative"), arg
    for chunk in (0, -4):
        assert _refused(lib, _fingerprint(lib, chunk=chunk), name, b"chunk"), chunk
    for arg in ("partial", "out"):
        assert _refused(lib, _fingerprint(lib, **{arg: None}), name, b"NULL pointer"), arg
    for which in (-1, 4):
        assert _refused(lib, _fingerprint(lib, which=which), name, b"which"), which
    assert _refused(lib, _fingerprint(lib, T=0, tensors=None, chunks=None, partial=None, out=None), name, b"NULL pointer (out)")


def test_nothing_to_pack_returns_without_a_launch(lib):
    """No tensors or no chunks: no table, no offsets and no bucket are needed, and nothing is launched (there is no
    device here to launch on).  The fingerprint's empty case writes its 0 on the device: tests/test_grad_bucket_gpu.py."""
    assert _pack(lib, T=0, tensors=None, chunks=None, offsets=None, bucket=None, numel=0) == 0
    assert _pack(lib, C=0, tensors=None, chunks=None, offsets=None, bucket=None, numel=0) == 0
    assert _pack(lib, T=0, C=0, zero=1, scale=1.0) == 0


def test_python_names_exist():
    from audio_motion_avatar_amd import dist, harness, ops, optim, triplane_net

    for name in ("bucket_offsets", "grads_pack", "tensors_fingerprint"):
        assert callable(getattr(ops, name)), name
    assert callable(optim.Adam.replicas_in_sync) and callable(dist.broadcast_module)
    for fn in (optim.Adam.__init__, optim.configure_optimizers, harness.AudioDrivenAvatar.configure_optimizers,
               triplane_net.TriplaneGaussianAvatar.configure_optimizers):
        assert inspect.signature(fn).parameters["process_group"].default is None, fn
    assert list(inspect.signature(dist.broadcast_module).parameters) == ["module", "src", "group", "buffers"]


def test_adam_with_a_group_refuses_host_parameters_as_before():
    import torch

    from audio_motion_avatar_amd import optim

    good = torch.nn.Parameter(torch.zeros(4))
    for backend in optim.BACKENDS:
        with pytest.raises(ValueError, match="parameter 0"):
            optim.Adam([good], backend=backend, process_group=object())      # refused before the group is looked at
