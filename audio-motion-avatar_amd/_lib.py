"""ctypes binding of libamav_hip.so, generated from include/amav.h: the header is parsed once at import and every
struct and prototype it declares becomes a ctypes.Structure / a SIGNATURES entry (the rules are parse_header's).

There is no CPU or eager fallback: if the library is missing, or an entry point fails, an exception is raised.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# AMAV_LIB: another build of the SAME library (tools/ablate_render.sh builds diagnostic variants of the blend kernel
# with -DAMAV_ABLATE=n); never a different implementation -- the symbol table is checked against include/amav.h either way
LIB_PATH = os.environ.get("AMAV_LIB") or os.path.join(_HERE, "csrc", "libamav_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "amav.h")

c_float_p = ctypes.c_void_p  # device pointers travel as integers (tensor.data_ptr())


class AmavError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "size_t": ctypes.c_size_t, "uint8_t": ctypes.c_uint8}
_RETURNS = {("int", ""): ctypes.c_int, ("int64_t", ""): ctypes.c_int64, ("size_t", ""): ctypes.c_size_t,
            ("char", "*"): ctypes.c_char_p}
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FIELD = re.compile(r"(?:const\s+)?(\w+)\s+(.+)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?")
_PROTOTYPE = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*\(([^()]*)\)")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*(\*{0,2})\s*(\w+)")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", re.M)


def _field_type(base, star, structs, decl):
    if star:
        if base in structs:
            return ctypes.POINTER(structs[base])
        if base == "void" or base in _SCALARS:
            return ctypes.c_void_p
    elif base in _SCALARS or base in structs:
        return _SCALARS.get(base) or structs[base]
    raise AmavError(f"amav.h: unknown type in struct field `{decl}`")


def _param_type(param, structs, decl):
    m = _PARAM.fullmatch(param)
    if not m:
        raise AmavError(f"amav.h: cannot read parameter `{param}` of `{decl}`")
    base, stars, name = m.groups()
    if not stars and base in _SCALARS:
        return _SCALARS[base]
    if stars == "*" and base == "char":
        return ctypes.c_char_p
    if stars == "*" and base in structs:
        return ctypes.POINTER(structs[base])
    if base == "void" and stars:
        return ctypes.c_void_p if stars == "*" else ctypes.POINTER(ctypes.c_void_p)
    if stars == "*" and base in _SCALARS:  # *_dev: a device address; anything else: a host out-parameter
        return ctypes.c_void_p if name.endswith("_dev") else ctypes.POINTER(_SCALARS[base])
    raise AmavError(f"amav.h: unknown type in parameter `{param}` of `{decl}`")


def _declarations(text, where):
    """The `;`-terminated declarations of `text`, stripped; text after the last `;` is a declaration that lacks its own."""
    *decls, rest = text.split(";")
    if rest.strip():
        raise AmavError(f"amav.h: missing `;` after `{' '.join(rest.split())}` in {where}")
    return [d.strip() for d in decls if d.strip()]


def parse_header(text):
    """C text of include/amav.h -> (structs: C name -> ctypes.Structure, signatures: name -> (restype, argtypes),
    defines: name -> int, the integer #defines; other preprocessor lines and comments are dropped).  A declaration that
    is not a `typedef struct` or a prototype over the types the header uses raises AmavError naming it: a new construct
    fails at import and never binds a wrong type."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {name: int(value) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
    if wrapped:
        text = text.rstrip()
        if not text.endswith("}"):
            raise AmavError('amav.h: `extern "C" {` is not closed')
        text = text[:-1]
    structs, signatures = {}, {}

    def struct(m):
        name, body = m.group(1), m.group(2)
        if m.group(3) != name:
            raise AmavError(f"amav.h: `typedef struct {name}` is named `{m.group(3)}`")
        fields = []
        for decl in _declarations(body, name):
            f = _FIELD.fullmatch(decl)
            declarators = [_DECLARATOR.fullmatch(d.strip()) for d in f.group(2).split(",")] if f else [None]
            if not all(declarators):
                raise AmavError(f"amav.h: cannot read struct field `{decl}` of {name}")
            for star, field, count in (d.groups() for d in declarators):
                ctype = _field_type(f.group(1), star, structs, decl)
                fields.append((field, ctype * int(count) if count else ctype))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return ""

    for decl in _declarations(_STRUCT.sub(struct, text), "the header"):
        m = _PROTOTYPE.fullmatch(decl)
        if not m or (m.group(1), m.group(2)) not in _RETURNS:
            raise AmavError(f"amav.h: cannot read declaration `{' '.join(decl.split())}`")
        params = [p.strip() for p in m.group(4).split(",")]
        argtypes = [] if params == ["void"] else [_param_type(p, structs, m.group(3)) for p in params]
        signatures[m.group(3)] = (_RETURNS[m.group(1), m.group(2)], argtypes)
    return structs, signatures, defines


def _load_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise AmavError(f"{HEADER_PATH}: cannot read the header the binding is generated from ({e})") from None


# name -> (restype, argtypes) of every symbol include/amav.h declares; its structs; its integer #defines
STRUCTS, SIGNATURES, DEFINES = _load_header()
Attr = STRUCTS["amav_attr"]  # element (f, i) at ptr[f * frame_stride + i * elem_stride] (strides in floats)
RasterArgs = STRUCTS["amav_raster_args"]
RasterBackwardArgs = STRUCTS["amav_raster_backward_args"]
ShArgs = STRUCTS["amav_sh_args"]
TriplaneDecodeBackwardArgs = STRUCTS["amav_triplane_decode_backward_args"]
TriplaneSampleBackwardArgs = STRUCTS["amav_triplane_sample_backward_args"]
DecodeSource = STRUCTS["amav_decode_source"]
BodyTables = STRUCTS["amav_body_tables"]
PoseParts = STRUCTS["amav_pose_parts"]
LbsBackwardArgs = STRUCTS["amav_lbs_backward_args"]
ImageView = STRUCTS["amav_image_view"]  # element (n, y, x, c) at ptr[n * image + y * row + x * pixel + c * channel stride]
ImageLossWindow = STRUCTS["amav_image_loss_window"]
Conv3x3Args = STRUCTS["amav_conv3x3_args"]
Conv3x3BackwardArgs = STRUCTS["amav_conv3x3_backward_args"]

_lib = None


def lib():
    """Load libamav_hip.so once.  Raises AmavError when it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AmavError(
                f"{LIB_PATH} is missing: the HIP extension is the only execution path of this package "
                "(no CPU fallback). Build it with `python -c 'import __graft_entry__ as g; g.build()'`.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError here = header and library out of sync
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().amav_last_error().decode("utf-8", "replace")
        raise AmavError(f"{what or 'amav call'} failed ({rc}): {msg}")
