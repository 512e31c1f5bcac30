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

The way back in: `parse_jpeg` reads a baseline JPEG's header segments into the record the device decoder takes
(ops.jpeg_decode); `AviReader`, `MjpegReader` and `DirReader` find the frames of an .avi, a bare .mjpeg and a directory of
frame_*.jpg; `load_clip` turns any of them into a device tensor with one upload and one decode call.  All of it is host
code on `struct` / `bytes`.
"""
import ctypes
import dataclasses
import os
import struct
from fractions import Fraction

from . import _lib, clip_io

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


# ------------------------------------------------------------------------------------------------------- JPEG headers
class JpegError(ValueError):
    """A JPEG the device decoder does not take (the message names the cause), or a frame it could not decode."""


# T.81 Annex K Huffman tables (K.3 - K.6): what a frame without any DHT segment means in an MJPG AVI
_K_DC_COUNTS = (bytes.fromhex("00010501010101010100000000000000"), bytes.fromhex("00030101010101010101010000000000"))
_K_DC_VALUES = bytes(range(12))
_K_AC_COUNTS = (bytes.fromhex("0002010303020403050504040000017d"), bytes.fromhex("00020102040403040705040400010277"))
_K_AC_VALUES = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
ANNEX_K_HUFFMAN = {(0, 0): (_K_DC_COUNTS[0], _K_DC_VALUES), (0, 1): (_K_DC_COUNTS[1], _K_DC_VALUES),
                   (1, 0): (_K_AC_COUNTS[0], _K_AC_VALUES[0]), (1, 1): (_K_AC_COUNTS[1], _K_AC_VALUES[1])}

_SOF_REFUSED = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
                0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
                0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10)",
                0xCB: "arithmetic coding (SOF11)", 0xCC: "arithmetic coding (DAC)", 0xCD: "arithmetic coding (SOF13)",
                0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


@dataclasses.dataclass
class JpegHeader:
    """What ops.jpeg_decode needs of one frame.  Per component (Y, Cb, Cr, or Y alone): its 64 quantisation entries in
    the file's zigzag order and its Huffman tables as the DHT (counts[16], values) pairs.  scan_begin / scan_end are
    byte offsets from the frame's SOI: the first byte after SOS, and the end of the frame (EOI included; the end of the
    data when there is no EOI, which the decoder reports in its status)."""
    height: int
    width: int
    components: int
    sampling: str               # "444", "420" or "gray"
    quant: list
    dc: list
    ac: list
    restart_interval: int       # MCUs, 0 = none
    scan_begin: int
    scan_end: int
    has_dht: bool
    has_eoi: bool
    segments: list              # marker bytes in order of appearance

    @property
    def geometry(self):
        return self.height, self.width, self.sampling


def _be16(data, at):
    return data[at] << 8 | data[at + 1]


def parse_jpeg(data, pos=0):
    """The header segments of the baseline JPEG that starts at data[pos] -> (JpegHeader, bytes consumed up to and
    including EOI).  Accepts SOF0, 8 bit, 1 or 3 components, 4:4:4 or 4:2:0, one interleaved sequential scan, 8-bit
    quantisation tables; anything else raises JpegError naming the cause."""
    if not isinstance(data, (bytes, bytearray)):
        data = bytes(data)
    size = len(data)
    if size - pos < 4 or data[pos] != 0xFF or data[pos + 1] != 0xD8:
        raise JpegError(f"no SOI marker at byte {pos}")
    at, quant, huffman, frame, ri, segments = pos + 2, {}, {}, None, 0, []
    while True:
        while at < size and data[at] == 0xFF and at + 1 < size and data[at + 1] == 0xFF:
            at += 1  # fill bytes
        if at + 4 > size:
            raise JpegError("the header ends before SOS")
        if data[at] != 0xFF or data[at + 1] in (0x00, 0xFF):
            raise JpegError(f"marker expected at byte {at - pos}")
        marker, n = data[at + 1], _be16(data, at + 2)
        if n < 2 or at + 2 + n > size:
            raise JpegError(f"segment {marker:02X} at byte {at - pos} overruns the data")
        body = bytes(data[at + 4:at + 2 + n])
        segments.append(marker)
        if marker in _SOF_REFUSED:
            raise JpegError(f"{_SOF_REFUSED[marker]} is not supported: baseline sequential (SOF0) only")
        if marker == 0xC0:
            if frame is not None:
                raise JpegError("a second SOF0 segment")
            if body[0] != 8:
                raise JpegError(f"{body[0]} bit samples are not supported: 8 bit only")
            height, width, nc = _be16(body, 1), _be16(body, 3), body[5]
            if nc == 4:
                raise JpegError("4 components (CMYK / YCCK) are not supported: 1 or 3 only")
            if nc not in (1, 3) or len(body) < 6 + 3 * nc:
                raise JpegError(f"{nc} components are not supported: 1 or 3 only")
            if height == 0 or width == 0:
                raise JpegError(f"size {width}x{height} (a height given by DNL is not supported)")
            frame = (height, width, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                                     for i in range(nc)])
        elif marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise JpegError("16-bit quantisation tables are not supported: 8-bit DQT only")
                if len(body) < 65:
                    raise JpegError("a DQT segment ends inside a table")
                quant[body[0] & 15], body = body[1:65], body[65:]
        elif marker == 0xC4:
            while body:
                if len(body) < 17 or len(body) < 17 + sum(body[1:17]):
                    raise JpegError("a DHT segment ends inside a table")
                k = sum(body[1:17])
                if body[0] >> 4 > 1 or body[0] & 15 > 3 or k > 256:
                    raise JpegError(f"DHT with class / id {body[0]:02X} or {k} codes")
                huffman[body[0] >> 4, body[0] & 15], body = (body[1:17], body[17:17 + k]), body[17 + k:]
        elif marker == 0xDD:
            ri = _be16(body, 0)
        elif marker == 0xDA:
            break
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            raise JpegError(f"unexpected marker {marker:02X} before SOS")
        at += 2 + n
    if frame is None:
        raise JpegError("SOS before SOF0")
    height, width, comps = frame
    ns = body[0]
    if ns != len(comps) or len(body) < 4 + 2 * ns:
        raise JpegError(f"a scan of {ns} of the {len(comps)} components: several scans are not supported, one "
                        "interleaved scan only")
    if bytes(body[1 + 2 * ns:4 + 2 * ns]) != b"\x00\x3f\x00":
        raise JpegError("spectral selection / successive approximation in SOS: one sequential scan only")
    scan = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
    if [c[0] for c in comps] != [s[0] for s in scan]:
        raise JpegError("the scan's components are not the frame's, in order")
    factors = [(h, v) for _, h, v, _ in comps]
    if len(comps) == 1:
        sampling = "gray"  # a scan of one component is not interleaved: its factors do not matter
    elif factors == [(1, 1)] * 3:
        sampling = "444"
    elif factors == [(2, 2), (1, 1), (1, 1)]:
        sampling = "420"
    else:
        raise JpegError("sampling factors " + " ".join(f"{h}x{v}" for h, v in factors) + " (4:2:2 and others) are not "
                        "supported: 4:4:4 and 4:2:0 only")
    tables = huffman or ANNEX_K_HUFFMAN
    q, dc, ac = [], [], []
    for (_, _, _, tq), (_, td, ta) in zip(comps, scan):
        if tq not in quant:
            raise JpegError(f"quantisation table {tq} is not defined")
        if (0, td) not in tables or (1, ta) not in tables:
            raise JpegError(f"Huffman table DC {td} / AC {ta} is not defined")
        q.append(quant[tq]), dc.append(tables[0, td]), ac.append(tables[1, ta])
    begin = at + 2 + n
    # inside entropy-coded data FF is followed by 00, RSTn or fill bytes only, so the first FF D9 is the EOI
    eoi = data.find(b"\xff\xd9", begin)
    has_eoi = eoi >= 0
    end = eoi + 2 if has_eoi else size
    header = JpegHeader(height, width, len(comps), sampling, q, dc, ac, ri, begin - pos, end - pos, bool(huffman), has_eoi,
                        segments)
    return header, end - pos


JpegFrame = _lib.STRUCTS["amav_jpeg_frame"]
JPEG_RECORD_BYTES = ctypes.sizeof(JpegFrame)


def pack_record(header, offset=0):
    """amav_jpeg_frame of a frame whose SOI lies at byte `offset` of the stream buffer."""
    rec = JpegFrame(scan_begin=offset + header.scan_begin, scan_end=offset + header.scan_end,
                    restart_interval=header.restart_interval)

    def rows(field, items):  # three rows of equal length, one per component; what a table leaves free stays zero
        n = len(field) // 3
        for c, row in enumerate(items):
            field[n * c:n * c + len(row)] = row

    rows(rec.quant, header.quant)
    rows(rec.dc_counts, [c for c, _ in header.dc])
    rows(rec.dc_values, [v[:16] for _, v in header.dc])
    rows(rec.ac_counts, [c for c, _ in header.ac])
    rows(rec.ac_values, [v for _, v in header.ac])
    return bytes(rec)


def frame_records(headers, offsets):
    """Parsed headers + the byte offset of every frame in the stream buffer -> ops.JpegRecords on the host.  The frames
    of one decode call share height, width, component count and sampling."""
    import torch

    from .ops import JpegRecords

    headers = list(headers)
    if not headers or len(headers) != len(offsets):
        raise JpegError("frame_records: one offset per header, at least one frame")
    for i, h in enumerate(headers):
        if h.geometry != headers[0].geometry:
            raise JpegError(f"frames of unequal geometry in one call: frame {i} is {h.width}x{h.height} {h.sampling}, frame 0 "
                            f"is {headers[0].width}x{headers[0].height} {headers[0].sampling}")
    table = bytearray(b"".join(pack_record(h, int(o)) for h, o in zip(headers, offsets)))
    return JpegRecords(torch.frombuffer(table, dtype=torch.uint8), headers[0].height, headers[0].width, headers[0].sampling)


# ------------------------------------------------------------------------------------------------------------ readers
class AviReader(clip_io.Reader):
    """Motion-JPEG AVI 1.0 -> frame bytes.  Walks the first RIFF 'AVI ' of the file: `hdrl` for the streams (fps from the
    video strh's rate / scale, size and 'MJPG' from its strf; PCM format from the audio strf), then `movi` chunk by
    chunk ('##dc' / '##db' of the video stream, '##wb' of the audio stream, even padding, LIST 'rec ' groups, JUNK).
    `idx1` is not read: writers disagree on what its offsets are relative to.  Only the chunk headers are read here;
    frame_bytes(i) reads one frame's payload.  An empty video chunk repeats the previous frame (a dropped frame)."""

    def __init__(self, source):
        self._own = not hasattr(source, "read")
        self.fh = open(source, "rb") if self._own else source
        self._base = 0 if self._own else self.fh.tell()
        self.fh.seek(0, os.SEEK_END)
        file_end = self.fh.tell() - self._base
        head = self._read(0, 12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError("not a RIFF 'AVI ' file")
        riff_end = min(8 + struct.unpack("<I", head[4:8])[0], file_end)
        self.width = self.height = 0
        self.rate, self.scale = 0, 1
        self.handler = self.compression = b""
        self.video_stream = self.audio_stream = None
        self.channels = self.sample_rate = self.sample_bits = 0
        self._frames, self._audio, self._streams = [], [], 0
        seen_movi = False
        for fourcc, kind, at, n in self._chunks(12, riff_end):
            if fourcc == b"LIST" and kind == b"hdrl":
                self._header_list(at, at + n)
            elif fourcc == b"LIST" and kind == b"movi" and not seen_movi:
                seen_movi = True
                self._movi(at, at + n)
        if self.video_stream is None:
            raise ValueError("the AVI has no video stream")
        if self.handler.upper() != b"MJPG" and self.compression.upper() != b"MJPG":
            raise ValueError(f"video stream is {self.compression!r} / {self.handler!r}, not MJPG")
        if not seen_movi:
            raise ValueError("the AVI has no 'movi' list")
        self.fps = self.rate / self.scale if self.scale else None

    def _read(self, at, n):
        self.fh.seek(self._base + at)
        return self.fh.read(n)

    def _chunks(self, at, end):
        """(fourcc, list kind or None, payload offset, payload bytes) of the chunks in [at, end): a LIST's payload starts
        after its kind; a size that overruns the parent is cut to it (a file whose sizes were never patched)."""
        while at + 8 <= end:
            head = self._read(at, 12)
            fourcc, n = head[:4], struct.unpack("<I", head[4:8])[0]
            n = min(n, end - at - 8)
            if fourcc in (b"LIST", b"RIFF") and n >= 4:
                yield fourcc, head[8:12], at + 12, n - 4
            else:
                yield fourcc, None, at + 8, n
            at += 8 + n + (n & 1)

    def _header_list(self, at, end):
        for fourcc, kind, p, n in self._chunks(at, end):
            if fourcc == b"LIST" and kind == b"strl":
                stream, self._streams, fcc = self._streams, self._streams + 1, None
                for cc, _, q, m in self._chunks(p, p + n):
                    body = self._read(q, min(m, 64))
                    if cc == b"strh" and len(body) >= 28:
                        fcc, handler = body[:4], body[4:8]
                        scale, rate = struct.unpack("<II", body[20:28])
                        if fcc == b"vids" and self.video_stream is None:
                            self.video_stream, self.handler, self.scale, self.rate = stream, handler, scale, rate
                    elif cc == b"strf" and fcc == b"vids" and self.video_stream == stream and len(body) >= 20:
                        self.width, height = struct.unpack("<ii", body[4:12])
                        self.height, self.compression = abs(height), body[16:20]
                    elif cc == b"strf" and fcc == b"auds" and self.audio_stream is None and len(body) >= 16:
                        tag, ch, sr, _, _, bits = struct.unpack("<HHIIHH", body[:16])
                        if tag == 1:  # PCM
                            self.audio_stream, self.channels, self.sample_rate, self.sample_bits = stream, ch, sr, bits

    def _movi(self, at, end):
        for fourcc, kind, p, n in self._chunks(at, end):
            if fourcc == b"LIST":
                if kind == b"rec ":
                    self._movi(p, p + n)
                continue
            if not fourcc[:2].isdigit():
                continue  # JUNK and whatever else
            stream, what = int(fourcc[:2]), fourcc[2:]
            if stream == self.video_stream and what in (b"dc", b"db"):
                if n:
                    self._frames.append((p, n))
                elif self._frames:
                    self._frames.append(self._frames[-1])
            elif stream == self.audio_stream and what == b"wb":
                self._audio.append((p, n))

    def frame_bytes(self, i):
        at, n = self._frames[i]
        return self._read(at, n)

    def read_audio(self):
        """(interleaved PCM bytes, channels, sample rate) of the first PCM stream, or None."""
        if self.audio_stream is None:
            return None
        return b"".join(self._read(at, n) for at, n in self._audio), self.channels, self.sample_rate

    def close(self):
        if self._own:
            self.fh.close()


class MjpegReader(clip_io.Reader):
    """The bare concatenation of JPEG files (.mjpeg).  Frame boundaries are not stored anywhere, so the file is read
    once and every frame's header parsed to find its EOI."""

    def __init__(self, path):
        with open(path, "rb") as fh:
            self._data = fh.read()
        self._frames, at = [], self._data.find(b"\xff\xd8")
        while at >= 0:
            header, used = parse_jpeg(self._data, at)
            self._frames.append((at, used))
            at = self._data.find(b"\xff\xd8", at + used)
        if not self._frames:
            raise ValueError(f"{path}: no JPEG frame")
        self.height, self.width = header.height, header.width

    def frame_bytes(self, i):
        at, n = self._frames[i]
        return self._data[at:at + n]


class DirReader(clip_io.Reader):
    """A directory of per-frame JPEG files, frame_000.jpg ... in numeric order (what --frames-dir writes); without such
    names, every *.jpg / *.jpeg in name order."""

    def __init__(self, path):
        import re

        names = sorted(os.listdir(path))
        numbered = sorted((int(m.group(1)), n) for n in names for m in [re.fullmatch(r"frame_(\d+)\.jpe?g", n)] if m)
        chosen = [n for _, n in numbered] or [n for n in names if n.lower().endswith((".jpg", ".jpeg"))]
        if not chosen:
            raise ValueError(f"{path}: no JPEG files")
        self._frames = [os.path.join(path, n) for n in chosen]
        self.height = self.width = None

    def frame_bytes(self, i):
        with open(self._frames[i], "rb") as fh:
            return fh.read()


def open_clip(path):
    """AviReader, MjpegReader or DirReader by what `path` is."""
    path = os.fspath(path)
    if os.path.isdir(path):
        return DirReader(path)
    return MjpegReader(path) if path.lower().endswith((".mjpeg", ".mjpg")) else AviReader(path)


def load_clip(path, frames=None, device="cuda", layout="chw_f32", check=True):
    """A clip on disk (.avi, .mjpeg, or a directory of frame_*.jpg; or an open reader) -> device tensor: fp32 [F,3,H,W]
    in [0, 1] (layout "chw_f32", the layout of `target_video`) or uint8 [F,H,W,3] ("hwc_u8").  `frames`: a range or a
    list of frame indices (default: all), e.g. range(0, n, 2) for the reference's stride-2 clips.  Only those frames'
    bytes are read; their headers are parsed on the host, then records and bytes go up in one copy and are decoded by one
    ops.jpeg_decode call.  check=True reads the status words back once and raises JpegError naming the frames the
    decoder flagged; check=False returns (tensor, status on the device) without synchronising."""
    import torch

    from . import ops

    picked, blobs = clip_io.read_frames(path, frames, open_clip)
    headers, offsets, at = [], [], 0
    for i, blob in zip(picked, blobs):
        try:
            headers.append(parse_jpeg(blob)[0])
        except JpegError as e:
            raise JpegError(f"frame {i}: {e}") from None
        offsets.append(at)
        at += len(blob)
    records = frame_records(headers, offsets)
    table_bytes = records.table.numel()
    host = torch.empty(table_bytes + at, dtype=torch.uint8)
    host[:table_bytes] = records.table
    host[table_bytes:] = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8)
    out, status = clip_io.decode_uploaded(host, table_bytes, device, lambda stream, table: ops.jpeg_decode(
        stream, ops.JpegRecords(table, records.height, records.width, records.sampling), layout=layout))
    if not check:
        return out, status
    names = [(ops.JPEG_STATUS_MARKERS, "markers"), (ops.JPEG_STATUS_ENTROPY, "entropy")]
    clip_io.raise_damaged(JpegError, picked, status, lambda s: "+".join(name for bit, name in names if s & bit))
    return out
