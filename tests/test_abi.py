"""The C-ABI library loads and exports every symbol include/amav.h declares; host-side argument checks answer with
error codes (no kernel is launched here: there is no GPU in this container)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from abi_support import HEADER, lib  # noqa: F401 (lib: fixture)


def header_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(amav_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from audio_motion_avatar_amd import _lib

    names = header_symbols()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/amav.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes binding and header disagree"


PROBE_KINDS = {ctypes.c_float: "f32", ctypes.c_int32: "i32", ctypes.c_int64: "i64", ctypes.c_size_t: "size", ctypes.c_uint8: "u8"}


def compiler_layout(structs, workdir):
    """{struct: sizeof} and {(struct, field): (offsetof, sizeof, kind)} as the host C compiler lays out include/amav.h:
    a generated program that includes the header itself prints them.  kind: the scalar type of the field (of its
    elements, for an array), "other" for pointers and nested structs."""
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang",
                           os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang"))
               if c and shutil.which(c)), None)
    assert cc is not None, "no host C compiler found: the struct layout cannot be checked"
    lines = ["#include <stdio.h>", '#include "amav.h"',
             '#define KIND(x) _Generic((x), float: "f32", int32_t: "i32", int64_t: "i64", size_t: "size", uint8_t: "u8", '
             'default: "other")', "int main(void) {"]
    for name, S in structs.items():
        lines.append(f'    printf("{name} - %zu 0 -\\n", sizeof({name}));')
        for field, ctype in S._fields_:
            member = f"(({name} *)0)->{field}"
            element = member + "[0]" if issubclass(ctype, ctypes.Array) else member
            lines.append(f'    printf("{name} {field} %zu %zu %s\\n", offsetof({name}, {field}), sizeof({member}), '
                         f"KIND({element}));")
    lines += ["    return 0;", "}", ""]
    src, exe = os.path.join(workdir, "layout_probe.c"), os.path.join(workdir, "layout_probe")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    subprocess.run([cc, "-std=c11", "-I", os.path.dirname(HEADER), src, "-o", exe], check=True)
    sizes, fields = {}, {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        name, field, a, b, kind = line.split()
        if field == "-":
            sizes[name] = int(a)
        else:
            fields[name, field] = (int(a), int(b), kind)
    return sizes, fields


def test_struct_layouts_match_the_header(lib, tmp_path):
    """ctypes lays every struct of the binding out as the C compiler lays out the header's: size of the struct, offset,
    size and scalar type of every field."""
    from audio_motion_avatar_amd import _lib

    aliases = (_lib.Attr, _lib.RasterArgs, _lib.RasterBackwardArgs, _lib.TriplaneDecodeBackwardArgs,
               _lib.TriplaneSampleBackwardArgs, _lib.DecodeSource, _lib.BodyTables, _lib.PoseParts, _lib.LbsBackwardArgs)
    assert len(set(aliases)) == 9 and set(aliases) <= set(_lib.STRUCTS.values())
    sizes, fields = compiler_layout(_lib.STRUCTS, str(tmp_path))
    checked = 0
    for name, S in _lib.STRUCTS.items():
        assert ctypes.sizeof(S) == sizes[name], name
        for field, ctype in S._fields_:
            d = getattr(S, field)
            element = ctype._type_ if issubclass(ctype, ctypes.Array) else ctype
            assert (d.offset, d.size, PROBE_KINDS.get(element, "other")) == fields[name, field], (name, field)
            checked += 1
    assert checked == len(fields) >= 100
    assert ctypes.sizeof(_lib.Attr) == 24 and ctypes.sizeof(_lib.BodyTables) == 16 + 8 * 8


@pytest.mark.parametrize("text", [
    "int amav_f(unsigned x, void *stream);",                               # a type the rules do not know
    "typedef struct demo_s { int32_t a; double b; } demo_s;",
    "int amav_f(int x, void *stream)\nint amav_g(void);",                   # a missing `;`
    "int amav_f(int x, void *stream)",
    "typedef struct demo_s { int32_t a; float b } demo_s;",
    "typedef struct demo_s { int32_t a; } demo_s\nint amav_f(void);",
    "int amav_f(void (*callback)(int), void *stream);",                    # a function-pointer parameter
    "typedef struct demo_s { void (*callback)(int); } demo_s;",
    "float amav_f(void);",                                                 # a return type no entry point has
    "int amav_f(amav_unknown *args, void *stream);",
    "typedef struct demo_s { float **rows; } demo_s;",
    "int amav_f(int);",                                                    # an unnamed parameter: no `_dev` rule to apply
    "int amav_limit = 3;",
])
def test_parser_refuses_what_it_does_not_recognise(text):
    from audio_motion_avatar_amd import AmavError, _lib

    with pytest.raises(AmavError, match="amav.h"):
        _lib.parse_header(text)


def test_parser_applies_the_binding_rules_to_text():
    from audio_motion_avatar_amd import _lib

    structs, signatures, defines = _lib.parse_header("""
        /* a comment with a prototype: int amav_hidden(void); */
        #define AMAV_N (-3)
        #ifdef __cplusplus
        extern "C" {
        #endif
        typedef struct demo_s { int32_t a, b[2]; const float *rows[3]; size_t n; } demo_s;  // trailing comment
        typedef struct demo_t { demo_s s; const demo_s *q; void *scratch; } demo_t;
        size_t amav_f(const demo_t *t, void **event, const char *name, const float *x_dev, float *ms, int64_t n, void *stream);
        const char *amav_g(void);
        #ifdef __cplusplus
        }
        #endif
    """)
    S, T = structs["demo_s"], structs["demo_t"]
    assert defines == {"AMAV_N": -3} and list(structs) == ["demo_s", "demo_t"]
    assert S._fields_ == [("a", ctypes.c_int32), ("b", ctypes.c_int32 * 2), ("rows", ctypes.c_void_p * 3), ("n", ctypes.c_size_t)]
    assert T._fields_ == [("s", S), ("q", ctypes.POINTER(S)), ("scratch", ctypes.c_void_p)]
    assert signatures == {
        "amav_f": (ctypes.c_size_t, [ctypes.POINTER(T), ctypes.POINTER(ctypes.c_void_p), ctypes.c_char_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_float), ctypes.c_int64, ctypes.c_void_p]),
        "amav_g": (ctypes.c_char_p, [])}


def test_a_missing_header_fails_loudly(monkeypatch):
    from audio_motion_avatar_amd import AmavError, _lib

    monkeypatch.setattr(_lib, "HEADER_PATH", "/nonexistent/include/amav.h")
    with pytest.raises(AmavError, match="/nonexistent/include/amav.h"):
        _lib._load_header()


def test_version_and_error_reporting(lib):
    assert lib.amav_version().startswith(b"amav-hip")
    assert lib.amav_rasterize_forward(None, None) == -1                      # AMAV_ERR_INVALID_ARG
    assert b"args is NULL" in lib.amav_last_error()
    assert lib.amav_rasterize_workspace_bytes(0, 10, 16, 16, 100) == 0       # rejected sizes
    assert lib.amav_rasterize_workspace_bytes(2, 100, 64, 64, 1000) > 2 * 100 * 64
    assert lib.amav_lbs_forward(1, None, None, None, None, None, None, 0, None) == -1
    assert lib.amav_triplane_project(0, 4, 4, None, 0, None, None, None) == -1
    assert lib.amav_frames_to_rgb8(3, None, None, None) == -1                # not a multiple of 4
    assert lib.amav_points_gather(1, 1, 1, None, None, None, None) == -1


def test_split_product_entry_points_validate_before_touching_the_device(lib):
    """Argument checks and size queries of the split-product entry points run on the host (no launch on a bad call)."""
    import ctypes

    from audio_motion_avatar_amd import _lib

    fake = 4096  # a non-NULL, 16-byte aligned address that is never dereferenced on these paths
    # operand split: k must be a multiple of 8, formats 0 / 1, fp16 exponent in range
    assert lib.amav_split_operand(4, 12, fake, 12, 0, 0, 0, fake, None) == -1 and b"multiple of 8" in lib.amav_last_error()
    assert lib.amav_split_operand(4, 16, fake, 16, 0, 7, 0, fake, None) == -1 and b"format" in lib.amav_last_error()
    assert lib.amav_split_operand(4, 16, fake, 16, 0, 1, 500, fake, None) == -1
    assert lib.amav_split_operand(4, 16, None, 16, 0, 0, 0, fake, None) == -1
    # GEGLU / residual-LayerNorm: exactly one of the fp32 and the split output
    assert lib.amav_geglu(4, 16, fake, 32, None, fake, fake, 0, None) == -1 and b"exactly one" in lib.amav_last_error()
    assert lib.amav_geglu(4, 16, fake, 32, None, None, None, 0, None) == -1
    assert lib.amav_add_layernorm(4, 512, 4, None, None, None, fake, fake, fake, fake, 1e-5, fake, fake, 0, 0, None) == -1
    assert b"exactly one" in lib.amav_last_error()
    assert lib.amav_add_layernorm(4, 512, 4, None, fake, None, fake, fake, fake, fake, 1e-5, fake, None, 0, 0, None) == -1
    assert b"add_bias without add" in lib.amav_last_error()
    # attention: all three bounds or none
    assert lib.amav_selfattn_forward_bounded(1, 64, 1, 64, fake, fake, fake, 64, fake, 64, 0.125, 1.0, 0.0, 1.0, fake, 1 << 30,
                                             None) == -1
    assert b"all three bounds" in lib.amav_last_error()
    # prepared operands: sizes = header + two fp16 parts of every entry
    assert lib.amav_subm_weights_split_bytes(27, 64, 128) == 256 + 27 * 64 * 128 * 2 * 2
    assert lib.amav_subm_weights_split_bytes(27, 48, 128) == 0 and lib.amav_subm_weights_split_bytes(0, 64, 64) == 0
    assert lib.amav_subm_prepare_weights_split(27, 64, 128, fake, fake, 16, None) == -3        # AMAV_ERR_WORKSPACE
    t = _lib.BodyTables()
    t.num_verts, t.num_joints, t.num_coeffs, t.skin_k = 10475, 55, 20, 4
    for name in ("v_template", "blend", "j_template", "j_dirs", "parents", "skin_idx", "skin_w"):
        setattr(t, name, fake)
    kb = 20 + 54 * 9  # 506 blend rows, padded to 512: 32 k-steps of 16 per 32-vertex tile
    assert lib.amav_lbs_blend_split_bytes(ctypes.byref(t)) == 256 + 328 * 32 * 2 * 3 * 512 * 2 and kb == 506
    assert lib.amav_lbs_prepare_blend_split(ctypes.byref(t), fake + 8, 1 << 30, None) == -1    # not 256-byte aligned


def test_product_refuses_to_run_without_a_device():
    """No CPU fallback: a CPU tensor is an error, not a slow path."""
    import torch

    from audio_motion_avatar_amd import AmavError, ops

    with pytest.raises(AmavError, match="only runs on an MI355X"):
        ops.lbs_forward({}, torch.zeros(1, 165), torch.zeros(1, 20))
    with pytest.raises(AmavError):
        ops.triplane_project(torch.zeros(1, 4, 12), torch.zeros(3, 4, 16), 2)


def test_missing_library_fails_loudly(monkeypatch):
    from audio_motion_avatar_amd import AmavError, _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libamav_hip.so")
    with pytest.raises(AmavError, match="no CPU fallback"):
        _lib.lib()
