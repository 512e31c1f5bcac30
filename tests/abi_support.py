"""Shared by the *_abi.py tests, which call the C entry points on the host only (every call is refused before a launch)."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "amav.h")
FAKE = 4096  # non-NULL, 16-byte aligned, never dereferenced on these paths
ERR_INVALID, ERR_WORKSPACE = -1, -3  # AMAV_ERR_INVALID_ARG, AMAV_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as entry
    from audio_motion_avatar_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        entry.build()
    return _lib.lib()
