"""Motion-JPEG in an AVI 1.0 container with PCM audio: the playable form of the demo's clip that needs no external
encoder (the frames are JPEG-encoded on the device by ops.jpeg_encode; this module is host code on `struct`).

    RIFF 'AVI '
      LIST 'hdrl'
        'avih'                                   main header
        LIST 'strl'  'strh' vids/MJPG  'strf' BITMAPINFOHEADER (biCompression 'MJPG', 24 bit)
        LIST 'strl'  'strh' auds       'strf' WAVEFORMATEX PCM          (with audio only)
      LIST 'movi'    '00dc' one JPEG per chunk, '01wb' PCM, interleaved: audio at most one second ahead of the video
      'idx1'         one entry per chunk, offsets relative to the 'movi' fourcc

Chunks are padded to even length; sizes and frame counts are patched on close().  AVI 1.0 sizes are 32 bit and players
stop trusting them at 2 GiB: a chunk that would take the file past that raises before it is written (OpenDML is out of
scope).  The audio is cut to the clip's duration, frames / fps (main2.py:370-378 muxes with `-shortest`).
"""
import struct
from fractions import Fraction

AVI_MAX_BYTES = (1 << 31) - 1
AVIF_HASINDEX, AVIF_ISINTERLEAVED, AVIIF_KEYFRAME = 0x10, 0x100, 0x10


def fps_fraction(fps):
    """fps as the exact fraction rate / scale of the stream header (24.0 -> 24 / 1, 29.97 -> 2997 / 100)."""
    fr = Fraction(str(float(fps))).limit_denominator(1_000_000)
    if fr <= 0:
        raise ValueError(f"fps {fps} is not positive")
    return fr.numerator, fr.denominator


def load_pcm16(path):
    """WAV file -> (interleaved little-endian 16-bit PCM bytes, channels, sample rate).  A 16-bit file's own samples
    pass through untouched; other widths are requantised from audio_frontend.load_wav's floats."""
    import wave

    with wave.open(str(path), "rb") as w:
        ch, width, sr, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
        raw = w.readframes(n)
    if width == 2:
        return raw, ch, sr
    from .audio_frontend import load_wav

    waveform, sr = load_wav(str(path))  # [channels, samples] in [-1, 1)
    pcm = (waveform.T.contiguous() * 32768.0).round().clamp(-32768, 32767).short()
    return pcm.numpy().astype("<i2").tobytes(), int(waveform.shape[0]), sr


class AviWriter:
    """`write_frame(jpeg_bytes)` appends one video frame; `close()` writes what is left of the audio, the index and the
    final sizes.  `audio`: None, or (pcm16 bytes, channels, sample_rate).  `target`: a path, or a seekable binary stream
    (left open).  `max_bytes` is the container's size limit (a test lowers it instead of writing 2 GiB)."""

    def __init__(self, target, height, width, fps, audio=None, max_bytes=AVI_MAX_BYTES):
        self.height, self.width = int(height), int(width)
        self.rate, self.scale = fps_fraction(fps)
        self.max_bytes = int(max_bytes)
        self.frames = 0
        self.closed = False
        self._own = not hasattr(target, "write")
        self.fh = open(target, "wb") if self._own else target
        self._base = self.fh.tell()
        self.audio = None
        if audio is not None:
            pcm, channels, sample_rate = audio
            self.channels, self.sample_rate = int(channels), int(sample_rate)
            self.block_align = 2 * self.channels
            self.audio = memoryview(bytes(pcm))[:len(pcm) // self.block_align * self.block_align]
        self._audio_at = 0      # bytes of PCM written
        self._index = []        # (fourcc, flags, offset from the 'movi' fourcc, payload bytes)
        self._max_frame = 0
        self._size = 0          # bytes of the file so far
        self._write_headers()

    # -- layout ------------------------------------------------------------------------------------------------
    def _headers(self, total_frames, audio_bytes, movi_bytes, max_frame):
        usec = round(1_000_000 * self.scale / self.rate)
        streams = 2 if self.audio is not None else 1
        bytes_per_sec = int(max_frame * self.rate / self.scale) + (self.sample_rate * self.block_align if self.audio is not None else 0)
        avih = struct.pack("<14I", usec, bytes_per_sec, 0, AVIF_HASINDEX | AVIF_ISINTERLEAVED, total_frames, 0, streams,
                           max_frame, self.width, self.height, 0, 0, 0, 0)
        strh_v = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, total_frames,
                             max_frame, 0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf_v = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3,
                             0, 0, 0, 0)
        strls = [_list(b"strl", _chunk(b"strh", strh_v) + _chunk(b"strf", strf_v))]
        if self.audio is not None:
            strh_a = struct.pack("<4s4sIHHIIIIIIII4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, self.block_align,
                                 self.sample_rate * self.block_align, 0, audio_bytes // self.block_align,
                                 self.sample_rate * self.block_align, 0xFFFFFFFF, self.block_align, 0, 0, 0, 0)
            strf_a = struct.pack("<HHIIHH", 1, self.channels, self.sample_rate, self.sample_rate * self.block_align,
                                 self.block_align, 16)
            strls.append(_list(b"strl", _chunk(b"strh", strh_a) + _chunk(b"strf", strf_a)))
        hdrl = _list(b"hdrl", _chunk(b"avih", avih) + b"".join(strls))
        movi_head = b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        return hdrl, movi_head

    def _write_headers(self):
        hdrl, movi_head = self._headers(0, 0, 0, 0)
        self.fh.write(b"RIFF" + struct.pack("<I", 0) + b"AVI " + hdrl + movi_head)
        self._movi_fourcc = 12 + len(hdrl) + 8  # file offset of the 'movi' fourcc
        self._size = self._movi_fourcc + 4

    def _append(self, fourcc, payload, flags):
        n = len(payload)
        # what the file would hold after this chunk and the index that then has to follow
        after = self._size + 8 + n + (n & 1) + 8 + 16 * (len(self._index) + 1)
        if after > self.max_bytes:
            raise ValueError(f"AVI 1.0 file would reach {after} bytes, past the {self.max_bytes}-byte limit, at frame "
                             f"{self.frames} (OpenDML is not supported: write shorter clips)")
        self._index.append((fourcc, flags, self._size - self._movi_fourcc, n))
        self.fh.write(fourcc + struct.pack("<I", n))
        self.fh.write(payload)
        if n & 1:
            self.fh.write(b"\0")
        self._size += 8 + n + (n & 1)

    def _audio_until(self, seconds):
        """PCM up to `seconds` of the track (a Fraction), in whole sample frames."""
        if self.audio is None:
            return
        end = min(int(seconds * self.sample_rate) * self.block_align, len(self.audio))
        if end > self._audio_at:
            self._append(b"01wb", self.audio[self._audio_at:end], AVIIF_KEYFRAME)
            self._audio_at = end

    # -- interface ---------------------------------------------------------------------------------------------
    def write_frame(self, jpeg):
        if self.closed:
            raise ValueError("AviWriter is closed")
        # audio leads by at most one second: before frame k goes everything up to (k / fps + 1 s), cut to the frames seen
        t = Fraction(self.frames * self.scale, self.rate)
        self._audio_until(min(t + 1, Fraction((self.frames + 1) * self.scale, self.rate)))
        self._append(b"00dc", jpeg, AVIIF_KEYFRAME)
        self.frames += 1
        self._max_frame = max(self._max_frame, len(jpeg))

    def close(self):
        if self.closed:
            return
        self.closed = True
        self._audio_until(Fraction(self.frames * self.scale, self.rate))  # the rest, cut to the clip's duration
        movi_bytes = self._size - self._movi_fourcc - 4
        idx = b"".join(fourcc + struct.pack("<III", flags, off, n) for fourcc, flags, off, n in self._index)
        self.fh.write(_chunk(b"idx1", idx))
        self._size += 8 + len(idx)
        hdrl, movi_head = self._headers(self.frames, self._audio_at, movi_bytes, self._max_frame)
        self.fh.seek(self._base)
        self.fh.write(b"RIFF" + struct.pack("<I", self._size - 8) + b"AVI " + hdrl + movi_head)
        self.fh.seek(self._base + self._size)
        if self._own:
            self.fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _chunk(fourcc, payload):
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def _list(kind, payload):
    return b"LIST" + struct.pack("<I", 4 + len(payload)) + kind + payload
