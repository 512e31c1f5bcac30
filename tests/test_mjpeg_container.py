"""mjpeg.AviWriter: the file is walked by an independent RIFF reader written here; the JPEGs are Pillow's."""
import io
import struct
from fractions import Fraction

import numpy as np
import pytest

import jpeg_cases as jc


def u32(data, at):
    return struct.unpack("<I", data[at:at + 4])[0]


def walk(data):
    """RIFF tree: [(fourcc, list kind or None, payload offset, payload size, children)]; asserts every size and the even
    padding: a chunk's successor starts at the next even offset, and a list ends exactly where its last child ends."""
    def chunks(at, end):
        out = []
        while at < end:
            assert at % 2 == 0, f"chunk at odd offset {at}"
            fourcc, n = data[at:at + 4], u32(data, at + 4)
            assert at + 8 + n <= end, f"{fourcc} at {at} overruns its parent"
            if fourcc in (b"RIFF", b"LIST"):
                out.append((fourcc, data[at + 8:at + 12], at + 12, n - 4, chunks(at + 12, at + 8 + n)))
            else:
                out.append((fourcc, None, at + 8, n, []))
                if n & 1:
                    assert data[at + 8 + n] == 0, "pad byte"
            at += 8 + n + (n & 1)
        assert at == end or at == end + 1
        return out

    tree = chunks(0, len(data))
    assert len(tree) == 1 and tree[0][0] == b"RIFF" and tree[0][1] == b"AVI " and u32(data, 4) == len(data) - 8
    return tree[0][4]


def find(children, fourcc, kind=None):
    return [c for c in children if c[0] == fourcc and c[1] == kind]


def check_avi(data, jpegs, height, width, fps, audio=None):
    top = walk(data)
    assert [(c[0], c[1]) for c in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl, movi, idx1 = top
    streams = find(hdrl[4], b"LIST", b"strl")
    assert len(streams) == (2 if audio else 1) and hdrl[4][0][0] == b"avih"
    avih = struct.unpack("<14I", data[hdrl[4][0][2]:hdrl[4][0][2] + 56])
    assert hdrl[4][0][3] == 56
    assert avih[4] == len(jpegs) and avih[6] == len(streams) and (avih[8], avih[9]) == (width, height)
    assert avih[3] & 0x10, "AVIF_HASINDEX"
    assert abs(avih[0] - 1e6 / fps) <= 1 and avih[7] >= max(len(j) for j in jpegs)
    # video stream
    strh, strf = streams[0][4]
    assert (strh[0], strh[3], strf[0], strf[3]) == (b"strh", 56, b"strf", 40)
    h = struct.unpack("<4s4sIHHIIIIIIII4H", data[strh[2]:strh[2] + 56])
    assert h[0] == b"vids" and h[1] == b"MJPG" and h[9] == len(jpegs)
    assert Fraction(h[7], h[6]) == Fraction(str(fps)), "rate / scale is the exact fps"
    assert h[-2:] == (width, height)
    b = struct.unpack("<IiiHH4sIiiII", data[strf[2]:strf[2] + 40])
    assert b[:6] == (40, width, height, 1, 24, b"MJPG")
    pcm_cut = b""
    if audio:
        pcm, channels, rate = audio
        strh, strf = streams[1][4]
        h = struct.unpack("<4s4sIHHIIIIIIII4H", data[strh[2]:strh[2] + 56])
        assert h[0] == b"auds" and Fraction(h[7], h[6]) == rate and h[12] == 2 * channels
        assert struct.unpack("<HHIIHH", data[strf[2]:strf[2] + 16]) == (1, channels, rate, rate * 2 * channels, 2 * channels, 16)
        samples = int(Fraction(len(jpegs)) / Fraction(str(fps)) * rate)
        pcm_cut = pcm[:samples * 2 * channels]
        assert h[9] == len(pcm_cut) // (2 * channels)
    # movi: the chunks, in order, and the index pointing at them
    assert all(c[0] in (b"00dc", b"01wb") for c in movi[4])
    video = [data[c[2]:c[2] + c[3]] for c in movi[4] if c[0] == b"00dc"]
    sound = b"".join(data[c[2]:c[2] + c[3]] for c in movi[4] if c[0] == b"01wb")
    assert video == list(jpegs)
    assert sound == pcm_cut
    movi_fourcc = movi[2] - 4
    assert idx1[3] == 16 * len(movi[4])
    for k, c in enumerate(movi[4]):
        fourcc, flags, off, n = struct.unpack("<4sIII", data[idx1[2] + 16 * k:idx1[2] + 16 * k + 16])
        assert (fourcc, n) == (c[0], c[3]) and flags & 0x10
        assert movi_fourcc + off == c[2] - 8, "idx1 offset is relative to the 'movi' fourcc"
        assert data[movi_fourcc + off:movi_fourcc + off + 4] == c[0]
    if audio:  # interleaving: audio never runs more than a second ahead of the video written so far
        frames_seen, bytes_seen = 0, 0
        for c in movi[4]:
            if c[0] == b"00dc":
                frames_seen += 1
            else:
                bytes_seen += c[3]
                assert Fraction(bytes_seen, 2 * audio[1] * audio[2]) <= Fraction(frames_seen) / Fraction(str(fps)) + 1
    return video


def jpegs_and_pcm(n, seconds=1.0, channels=1, rate=8000):
    frames = jc.noise(n, 16, 24, seed=5)
    jpegs = [jc.pillow_jpeg(f, 60 + i, "420", 1) for i, f in enumerate(frames)]
    assert any(len(j) & 1 for j in jpegs) and any(not len(j) & 1 for j in jpegs), "both parities, for the padding"
    pcm = np.random.default_rng(1).integers(-30000, 30000, int(seconds * rate) * channels).astype("<i2").tobytes()
    return jpegs, pcm


@pytest.mark.parametrize("fps", [24.0, 29.97, 12.5])
@pytest.mark.parametrize("channels", [0, 1, 2])
def test_avi_layout(tmp_path, fps, channels):
    from audio_motion_avatar_amd.mjpeg import AviWriter

    jpegs, pcm = jpegs_and_pcm(9, seconds=1.0, channels=max(channels, 1))
    audio = (pcm, channels, 8000) if channels else None
    path = tmp_path / "clip.avi"
    with AviWriter(str(path), 16, 24, fps, audio=audio) as w:
        for j in jpegs:
            w.write_frame(j)
    assert w.frames == 9
    check_avi(path.read_bytes(), jpegs, 16, 24, fps, audio)


def test_avi_audio_shorter_than_the_clip_and_streams(tmp_path):
    """A track that ends before the video is written whole; a seekable stream works like a path and stays open."""
    from audio_motion_avatar_amd.mjpeg import AviWriter

    jpegs, pcm = jpegs_and_pcm(30, seconds=0.5)
    buf = io.BytesIO()
    w = AviWriter(buf, 16, 24, 24.0, audio=(pcm, 1, 8000))
    for j in jpegs:
        w.write_frame(j)
    w.close()
    w.close()  # idempotent
    assert not buf.closed
    top = walk(buf.getvalue())
    sound = b"".join(buf.getvalue()[c[2]:c[2] + c[3]] for c in top[1][4] if c[0] == b"01wb")
    assert sound == pcm
    with pytest.raises(ValueError, match="closed"):
        w.write_frame(jpegs[0])


def test_avi_refuses_to_grow_past_its_limit(tmp_path):
    """The 2 GiB rule through a lowered limit: the chunk that would cross it raises before anything of it is written,
    and the file closed after that is whole."""
    from audio_motion_avatar_amd import mjpeg

    assert mjpeg.AVI_MAX_BYTES == 2 ** 31 - 1
    jpegs, _ = jpegs_and_pcm(9)
    path = tmp_path / "clip.avi"
    w = mjpeg.AviWriter(str(path), 16, 24, 24.0, max_bytes=4000)
    written = []
    with pytest.raises(ValueError, match="AVI 1.0.*4000-byte limit.*OpenDML"):
        for j in jpegs:
            w.write_frame(j)
            written.append(j)
    assert 0 < len(written) < len(jpegs)
    w.close()
    data = path.read_bytes()
    assert len(data) <= 4000
    check_avi(data, written, 16, 24, 24.0)
    # one more chunk of that size would not have fitted
    assert len(data) + 8 + len(jpegs[len(written)]) + 16 > 4000


def test_pcm16_passes_16_bit_files_through_and_requantises_the_rest(tmp_path):
    import wave

    from audio_motion_avatar_amd.mjpeg import load_pcm16

    pcm = np.random.default_rng(2).integers(-32768, 32767, 400).astype("<i2")
    with wave.open(str(tmp_path / "a.wav"), "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(22050)
        w.writeframes(pcm.tobytes())
    assert load_pcm16(tmp_path / "a.wav") == (pcm.tobytes(), 2, 22050)
    with wave.open(str(tmp_path / "b.wav"), "wb") as w:  # 8 bit unsigned -> (v - 128) * 256
        w.setnchannels(1), w.setsampwidth(1), w.setframerate(8000)
        w.writeframes(bytes([0, 64, 128, 192, 255]))
    raw, ch, sr = load_pcm16(tmp_path / "b.wav")
    assert (ch, sr) == (1, 8000) and list(np.frombuffer(raw, dtype="<i2")) == [-32768, -16384, 0, 16384, 32512]


def test_fps_fraction():
    from audio_motion_avatar_amd.mjpeg import fps_fraction

    assert fps_fraction(24.0) == (24, 1) and fps_fraction(29.97) == (2997, 100) and fps_fraction(12.5) == (25, 2)
    with pytest.raises(ValueError):
        fps_fraction(0)
