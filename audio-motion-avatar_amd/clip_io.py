"""What the clip loaders of mjpeg.py and png.py share: the reader base class, picking and reading the frames, the one
upload with the records first, and the status read-back.  Host only: torch is imported where it is needed, so the
modules that parse files stay importable without the library."""


class Reader:
    """A clip as a sequence of per-frame file contents.  A subclass fills `_frames` and implements frame_bytes(i)."""
    fps = None

    def __len__(self):
        return len(self._frames)

    def frame_bytes(self, i):
        raise NotImplementedError

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_frames(source, frames, opener):
    """(picked indices, their file contents) of `source`: an open reader, which stays open, or what `opener` makes a
    reader of, which is closed again.  `frames`: indices (default: all)."""
    reader = source if hasattr(source, "frame_bytes") else opener(source)
    try:
        count = len(reader)
        picked = list(range(count)) if frames is None else [int(i) for i in frames]
        if not picked:
            raise ValueError("load_clip: no frames selected")
        for i in picked:
            if not -count <= i < count:
                raise IndexError(f"load_clip: frame {i} of a clip of {count}")
        return picked, [reader.frame_bytes(i) for i in picked]
    finally:
        if reader is not source:
            reader.close()


def decode_uploaded(host, table_bytes, device, decode):
    """The one upload of a clip: `host` holds the records (8-byte aligned, so they come first) and then the stream.
    Returns decode(stream, table), both views of the device copy: (frames, status)."""
    dev = host.to(device)
    return decode(dev[table_bytes:], dev[:table_bytes])


def raise_damaged(error, picked, status, text):
    """Read the status words back (one synchronisation) and raise `error` naming the frames the decoder flagged."""
    bad = [(i, s) for i, s in zip(picked, status.cpu().tolist()) if s]
    if bad:
        raise error("load_clip: damaged frames " + ", ".join(f"{i} ({text(s)})" for i, s in bad))
