"""mjpeg.AviReader / MjpegReader / DirReader: what AviWriter wrote comes back, hand-built AVIs of other writers' habits
are read, and frame selection reads only the chosen frames.  Host code only; the JPEGs are Pillow's."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_cases as jc


def jpegs_and_pcm(n, channels=1, rate=8000, seconds=1.0):
    frames = jc.noise(n, 16, 24, seed=5)
    jpegs = [jc.pillow_jpeg(f, 60 + i, "420", 1) for i, f in enumerate(frames)]
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs), "both parities, for the padding"
    pcm = np.random.default_rng(1).integers(-30000, 30000, int(seconds * rate) * channels).astype("<i2").tobytes()
    return jpegs, pcm


@pytest.mark.parametrize("fps", [24.0, 29.97])
@pytest.mark.parametrize("channels", [0, 1, 2])
def test_reads_back_what_the_writer_wrote(tmp_path, fps, channels):
    from audio_motion_avatar_amd.mjpeg import AviReader, AviWriter, fps_fraction

    jpegs, pcm = jpegs_and_pcm(9, channels=max(channels, 1))
    path = tmp_path / "clip.avi"
    with AviWriter(str(path), 16, 24, fps, audio=(pcm, channels, 8000) if channels else None) as w:
        for j in jpegs:
            w.write_frame(j)
    with AviReader(str(path)) as r:
        assert len(r) == 9 and (r.height, r.width) == (16, 24)
        assert (r.rate, r.scale) == fps_fraction(fps) and r.fps == pytest.approx(fps)
        assert [r.frame_bytes(i) for i in range(9)] == jpegs
        assert r.frame_bytes(-1) == jpegs[-1]
        if channels:
            samples = int(9 / fps * 8000)  # the writer cuts the track to the clip's duration
            assert r.read_audio() == (pcm[:samples * 2 * channels], channels, 8000)
            assert r.sample_bits == 16
        else:
            assert r.read_audio() is None


def chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def lst(kind, payload):
    return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload


def hand_built(jpegs, pcm, index="movi", rec=True, junk=True, stream_order=("auds", "vids"), db=False):
    """An AVI as other writers lay it out: the audio stream first (so video is '01dc'), frames grouped in LIST 'rec ',
    JUNK chunks before and inside movi, odd-sized chunks padded, '##db' for a frame, an idx1 whose offsets are file
    offsets (index="file"), offsets from the movi fourcc ("movi"), or no idx1 at all (None)."""
    strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"mjpg", 0, 0, 0, 0, 1001, 30000, 0, len(jpegs), 0, 0xFFFFFFFF, 0, 0, 0,
                         24, 16)
    strf_v = struct.pack("<IiiHH4sIiiII", 40, 24, 16, 1, 24, b"MJPG", 24 * 16 * 3, 0, 0, 0, 0)
    strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 2, 16000, 0, len(pcm) // 2, 0, 0xFFFFFFFF, 2,
                         0, 0, 0, 0)
    strf_a = struct.pack("<HHIIHH", 1, 1, 8000, 16000, 2, 16)
    strl = {"vids": lst(b"strl", chunk(b"strh", strh_v) + chunk(b"strf", strf_v) + chunk(b"strn", b"camera\0")),
            "auds": lst(b"strl", chunk(b"strh", strh_a) + chunk(b"strf", strf_a))}
    avih = struct.pack("<14I", 33367, 0, 0, 0x10, len(jpegs), 0, 2, 0, 24, 16, 0, 0, 0, 0)
    hdrl = lst(b"hdrl", chunk(b"avih", avih) + b"".join(strl[s] for s in stream_order) + (chunk(b"JUNK", bytes(37)) if junk else b""))
    v = b"%02ddc" % stream_order.index("vids")
    a = b"%02dwb" % stream_order.index("auds")
    third = len(pcm) // 3 // 2 * 2
    pieces = [chunk(a, pcm[:third])]
    for i, j in enumerate(jpegs):
        fourcc = v[:2] + b"db" if db and i == 1 else v
        group = chunk(fourcc, j) + (chunk(a, pcm[third:2 * third]) if i == 0 else b"")
        pieces.append(lst(b"rec ", group) if rec else group)
        if junk and i == 2:
            pieces.append(chunk(b"JUNK", bytes(11)))
    pieces.append(chunk(a, pcm[2 * third:]))
    movi = lst(b"movi", b"".join(pieces))
    head = b"RIFF" + bytes(4) + b"AVI " + hdrl + (chunk(b"JUNK", bytes(101)) if junk else b"")
    body = head + movi
    if index:
        # one entry per frame; what the offsets are relative to differs between writers, and these are made up anyway
        base = 0 if index == "file" else len(head) + 8
        body += chunk(b"idx1", b"".join(v + struct.pack("<III", 0x10, 12345 + 2 * i - base, len(j)) for i, j in enumerate(jpegs)))
    body = body[:4] + struct.pack("<I", len(body) - 8) + body[8:]
    return body + b"RIFF" + struct.pack("<I", 4) + b"AVIX"  # a second RIFF is not read


@pytest.mark.parametrize("index", ["movi", "file", None])
@pytest.mark.parametrize("rec", [True, False])
def test_reads_other_writers_layouts(tmp_path, index, rec):
    from audio_motion_avatar_amd.mjpeg import AviReader

    jpegs, pcm = jpegs_and_pcm(5, seconds=0.25)
    data = hand_built(jpegs, pcm, index=index, rec=rec, db=True)
    path = tmp_path / "other.avi"
    path.write_bytes(data)
    for source in (str(path), io.BytesIO(data)):
        r = AviReader(source)
        assert len(r) == 5 and [r.frame_bytes(i) for i in range(5)] == jpegs
        assert (r.height, r.width, r.rate, r.scale) == (16, 24, 30000, 1001) and r.fps == pytest.approx(29.97, abs=1e-3)
        assert (r.video_stream, r.audio_stream) == (1, 0)
        assert r.read_audio() == (pcm, 1, 8000)
        r.close()


def test_refuses_what_is_not_a_motion_jpeg_avi(tmp_path):
    from audio_motion_avatar_amd.mjpeg import AviReader

    jpegs, pcm = jpegs_and_pcm(3, seconds=0.1)
    data = hand_built(jpegs, pcm)
    with pytest.raises(ValueError, match="not a RIFF 'AVI ' file"):
        AviReader(io.BytesIO(b"RIFF" + bytes(4) + b"WAVE" + data[12:]))
    with pytest.raises(ValueError, match="not MJPG"):
        AviReader(io.BytesIO(data.replace(b"MJPG", b"H264").replace(b"mjpg", b"h264")))


def test_a_file_cut_short_gives_the_frames_that_are_whole(tmp_path):
    """Sizes that overrun the file (a recording that was never closed) are cut to it."""
    from audio_motion_avatar_amd.mjpeg import AviReader

    jpegs, pcm = jpegs_and_pcm(5, seconds=0.25)
    data = hand_built(jpegs, pcm, index=None, rec=False, junk=False)
    data = data[:data.index(jpegs[3]) + 10]
    r = AviReader(io.BytesIO(data))
    assert len(r) == 4 and [r.frame_bytes(i) for i in range(3)] == jpegs[:3] and r.frame_bytes(3) == jpegs[3][:10]


class CountingReader:
    """Wraps a reader and notes which frames were asked for."""

    def __init__(self, inner):
        self.inner, self.asked = inner, []

    def __len__(self):
        return len(self.inner)

    def frame_bytes(self, i):
        self.asked.append(i)
        return self.inner.frame_bytes(i)


def test_mjpeg_and_directory_readers(tmp_path):
    from audio_motion_avatar_amd.mjpeg import AviReader, DirReader, MjpegReader, open_clip

    jpegs, _ = jpegs_and_pcm(12)
    bare = tmp_path / "clip.mjpeg"
    bare.write_bytes(b"".join(jpegs))
    r = MjpegReader(str(bare))
    assert len(r) == 12 and [r.frame_bytes(i) for i in range(12)] == jpegs and (r.height, r.width) == (16, 24)
    frames_dir = tmp_path / "frames"
    os.makedirs(frames_dir)
    for i, j in enumerate(jpegs):  # frame_10 sorts before frame_2 by name, not by number
        (frames_dir / f"frame_{i}.jpg").write_bytes(j)
    (frames_dir / "notes.txt").write_text("not a frame")
    d = DirReader(str(frames_dir))
    assert len(d) == 12 and [d.frame_bytes(i) for i in range(12)] == jpegs
    assert isinstance(open_clip(str(bare)), MjpegReader) and isinstance(open_clip(frames_dir), DirReader)
    with pytest.raises(ValueError, match="not a RIFF"):
        open_clip(str(frames_dir / "notes.txt"))
    with pytest.raises(ValueError, match="no JPEG"):
        DirReader(str(tmp_path))
    assert AviReader is not None


def test_load_clip_reads_only_the_selected_frames(tmp_path, monkeypatch):
    """frames= as a range and as a list: only those frames' bytes are read, in that order, parsed, and handed to one
    decode call with one record per frame (the decode itself is replaced: this is the host side)."""
    import torch

    from audio_motion_avatar_amd import mjpeg, ops

    jpegs, pcm = jpegs_and_pcm(9)
    path = tmp_path / "clip.avi"
    with mjpeg.AviWriter(str(path), 16, 24, 24.0, audio=(pcm, 1, 8000)) as w:
        for j in jpegs:
            w.write_frame(j)
    calls = []

    def fake_decode(stream, records, layout="chw_f32", out=None, status=None):
        calls.append((bytes(stream.numpy()), records, layout))
        return torch.zeros(records.num_frames, 3, records.height, records.width), torch.zeros(records.num_frames, dtype=torch.int32)

    monkeypatch.setattr(ops, "jpeg_decode", fake_decode)
    for frames, want in ((range(0, 9, 2), [0, 2, 4, 6, 8]), ([7, 1, 1], [7, 1, 1]), (None, list(range(9))), ([-1], [-1])):
        calls.clear()
        reader = mjpeg.AviReader(str(path))
        counting = CountingReader(reader)
        out = mjpeg.load_clip(counting, frames=frames, device="cpu")
        reader.close()
        assert counting.asked == want and out.shape == (len(want), 3, 16, 24) and len(calls) == 1
        stream, records, layout = calls[0]
        assert stream == b"".join(jpegs[i] for i in want) and layout == "chw_f32"
        assert (records.num_frames, records.height, records.width, records.sampling) == (len(want), 16, 24, "420")
        at = 0
        for k, i in enumerate(want):
            begin, end = struct.unpack("<qq", bytes(records.table[k * 1128:k * 1128 + 16].numpy()))
            h = mjpeg.parse_jpeg(jpegs[i])[0]
            assert (begin, end) == (at + h.scan_begin, at + len(jpegs[i]))
            at += len(jpegs[i])
    with pytest.raises(IndexError, match="frame 9 of a clip of 9"):
        mjpeg.load_clip(str(path), frames=[9], device="cpu")
    with pytest.raises(mjpeg.JpegError, match="damaged frames 2 \\(entropy\\), 4 \\(markers\\+entropy\\)"):
        monkeypatch.setattr(ops, "jpeg_decode", lambda s, r, layout="chw_f32": (None, torch.tensor([0, 2, 3], dtype=torch.int32)))
        mjpeg.load_clip(str(path), frames=[0, 2, 4], device="cpu")
