"""ctypes binding of libduodiff.so, derived at import from include/duodiff.h and include/duodiff_dev.h: the two headers are the only
declaration of the ABI.  Every DD_* constant, every argument struct and SIGNATURES (name -> (restype, argtypes)) below come from their
text; a declaration outside the small subset of C they use raises HeaderError, quoting it.  No CPU fallback: a missing library is an
ImportError-class failure raised at first use, loudly."""
import ctypes as C
import os
import re
from pathlib import Path

LIB_PATH = Path(os.environ.get("DUODIFF_LIB") or Path(__file__).resolve().parent / "libduodiff.so")
INCLUDE = Path(__file__).resolve().parent.parent / "include"


class EngineUnavailable(RuntimeError):
    """libduodiff.so (or a header it is bound from) is missing or unusable.  There is no CPU path to fall back to."""


class HeaderError(ValueError):
    """a declaration of the headers that the binding does not derive a type for"""


SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
           "uint64_t": C.c_uint64, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "unsigned short": C.c_ushort,
           "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}


def _ctype(base, stars, types, field, host_rows, decl):
    """the ctypes type of `stars` pointers to `base`; types: struct name -> its class, or None for an opaque handle"""
    if base not in SCALARS and base not in types and base not in ("void", "char"):
        raise HeaderError(f"unknown type {base!r} in: {decl}")
    if stars == 0:
        if base not in SCALARS:
            raise HeaderError(f"{base!r} by value in: {decl}")
        return SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and types.get(base) is not None:
        return C.POINTER(types[base])
    # a scalar pointer field that is not *_dev is one of the public header's "host [n_steps]" arrays; every other pointer is an address
    return C.POINTER(SCALARS[base]) if field and host_rows and stars == 1 and base in SCALARS else C.c_void_p


def _declare(decl, types, field, dev, quote=None):
    """[(name, ctype)] of one field line (several declarators allowed) or one parameter (an array is a pointer); errors quote `quote`"""
    decl, quote = decl.strip(), quote or decl.strip()
    if "(" in decl:
        raise HeaderError(f"function pointer in: {quote}")
    if ":" in decl:
        raise HeaderError(f"bit-field in: {quote}")
    if re.search(r"[{}]|\b(struct|union|enum)\b", decl):
        raise HeaderError(f"nested or anonymous struct in: {quote}")
    out, base = [], None
    for piece in re.sub(r"\bconst\b", " ", decl).split(","):
        m = re.fullmatch(r"([\w\s*]*?)(\w+)\s*(\[\w*\])?", piece.strip())
        if not m:
            raise HeaderError(f"cannot read the declarator {piece.strip()!r} in: {quote}")
        prefix, name, array = m.groups()
        if array and field:
            raise HeaderError(f"array field in: {quote}")
        if base is None:
            base = " ".join(prefix.replace("*", " ").split())
        elif prefix.replace("*", "").strip():
            raise HeaderError(f"cannot read the declarator {piece.strip()!r} in: {quote}")
        out.append((name, _ctype(base, prefix.count("*") + bool(array), types, field, not dev and not name.endswith("_dev"), quote)))
    return out


def parse_header(text, dev=False, types=None):
    """(constants, types, signatures) of one header's text; types continues the dict of the headers read before it.  dev: the header
    is duodiff_dev.h, whose structs hold no host row arrays."""
    constants, types, signatures = {}, {} if types is None else types, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*", "", text, flags=re.S | re.M)     # extern "C" { ... }
    for line in re.findall(r"^[ \t]*#[^\n]*", text, flags=re.M):
        m = re.fullmatch(r"#\s*define\s+(DD_\w+)\b\s*(.*)", line.strip())
        if m:
            if not re.fullmatch(r"-?\d+[uU]?", m.group(2).strip()):
                raise HeaderError(f"not an integer constant: {line.strip()}")
            constants[m.group(1)] = int(m.group(2).strip().rstrip("uU"))
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    depth, start, statements = 0, 0, []
    for i, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            statements.append(" ".join(text[start:i].split()))
            start = i + 1
    if text[start:].strip():
        raise HeaderError(f"unfinished declaration: {' '.join(text[start:].split())}")
    for st in statements:
        if m := re.fullmatch(r"typedef struct (\w+) (\w+)", st):
            types.setdefault(m.group(1), None)
        elif m := re.fullmatch(r"(?:typedef )?enum \w*\s*\{(.*)\}\s*\w*", st):
            for item in filter(None, (s.strip() for s in m.group(1).split(","))):
                if not (e := re.fullmatch(r"(DD_\w+) = (-?\d+)", item)):
                    raise HeaderError(f"enumerator without an integer value {item!r} in: {st}")
                constants[e.group(1)] = int(e.group(2))
        elif m := re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", st):
            if m.group(1) != m.group(3) or "{" in m.group(2):
                raise HeaderError(f"nested or anonymous struct in: {st}")
            fields = [f for d in m.group(2).split(";") if d.strip() for f in _declare(d, types, True, dev)]
            types[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        elif (m := re.fullmatch(r"([\w\s*]+?)\b(dd_\w+)\s*\((.*)\)", st)) and "(" not in m.group(3):
            ret, params = re.sub(r"\bconst\b", " ", m.group(1)), m.group(3).strip()
            res = None if ret.split() == ["void"] else _ctype(" ".join(ret.replace("*", " ").split()), ret.count("*"), types, False, False, st)
            signatures[m.group(2)] = (res, [] if params == "void" else [_declare(p, types, False, dev, st)[0][1] for p in params.split(",")])
        else:
            raise HeaderError(f"{'function pointer in' if '(*' in st else 'cannot read'}: {st}")
    return constants, types, signatures


def _bind():
    """every DD_* constant and struct class becomes a module attribute; SIGNATURES holds every prototype of both headers"""
    types = {}
    for name, dev in (("duodiff.h", False), ("duodiff_dev.h", True)):
        if not (INCLUDE / name).exists():
            raise EngineUnavailable(f"{INCLUDE / name} not found: duodiff_amd binds libduodiff.so from the headers of its own tree")
        constants, types, signatures = parse_header((INCLUDE / name).read_text(), dev, types)
        globals().update(constants)
        SIGNATURES.update(signatures)
    globals().update({k: v for k, v in types.items() if v is not None})


SIGNATURES = {}
_bind()
ABI_VERSION = DD_ABI_VERSION  # noqa: F821  (bound from duodiff.h just above)

_lib = None


def load():
    """dlopen the in-tree library and attach prototypes.  Raises EngineUnavailable if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise EngineUnavailable(
            f"{LIB_PATH} not found: build it with `python -m duodiff_amd.build` "
            "(hipcc --offload-arch=gfx950).  duodiff_amd has no CPU fallback.")
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:  # e.g. libamdhip64 missing
        raise EngineUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    lib.dd_abi_version.restype = C.c_int
    if lib.dd_abi_version() != ABI_VERSION:
        raise EngineUnavailable(f"{LIB_PATH}: ABI version {lib.dd_abi_version()}, this package binds version {ABI_VERSION}; rebuild")
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # the production surface (include/duodiff.h) must be complete; a library built without the development entry
            # points (include/duodiff_dev.h: dd_dev_*), e.g. an A/B build of an older tree, still loads
            if name.startswith("dd_dev_"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
