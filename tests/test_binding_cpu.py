"""CPU: the ctypes binding duodiff_amd/_lib.py derives from include/duodiff.h and include/duodiff_dev.h -- the struct layouts against a C
compiler, the parser construct by construct on inline snippets, the longest prototypes pinned position by position, and the built library."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from conftest import REPO
from duodiff_amd import _lib as L

HEADERS = [(REPO / "include" / "duodiff.h").read_text(), (REPO / "include" / "duodiff_dev.h").read_text()]
STRUCTS = {k: v for k, v in vars(L).items() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}


def _c_compiler():
    """cc, else the clang that hipcc drives; the layout test fails without one"""
    from duodiff_amd.build import hipcc
    cands = [shutil.which("cc")]
    try:
        rocm_bin = Path(hipcc()).resolve().parent
        cands += [rocm_bin / "clang", rocm_bin.parent / "llvm" / "bin" / "clang", rocm_bin.parent / "lib" / "llvm" / "bin" / "clang"]
    except RuntimeError:
        pass
    for c in cands:
        if c and Path(c).exists():
            return str(c)
    pytest.fail("no C compiler (cc, or the clang beside hipcc): the derived struct layouts cannot be checked against one")


def test_struct_layouts_equal_the_compilers(tmp_path):
    """sizeof of every derived struct, offsetof and size of every field: what ctypes lays out is what a C compiler lays out from the headers"""
    assert len(STRUCTS) == sum(len(re.findall(r"typedef struct \w+ \{", h)) for h in HEADERS) >= 18
    prog, want = ['#include <stdio.h>', '#include "duodiff_dev.h"', "int main(void) {"], []
    for name, cls in STRUCTS.items():
        prog.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for f, _ in cls._fields_:
            prog.append(f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
            want.append(f"{name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}")
    (tmp_path / "layout.c").write_text("\n".join(prog + ["    return 0;", "}"]) + "\n")
    subprocess.run([_c_compiler(), "-x", "c", "-std=c11", f"-I{REPO / 'include'}", str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True, capture_output=True, text=True)
    got = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(want) >= 256 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_nothing_in_the_headers_is_left_out():
    """counted by plain searches of the header text: every DD_* value, every struct and every prototype is in the module"""
    consts = {k for k, v in vars(L).items() if k.startswith("DD_") and isinstance(v, int)}
    named = set()
    for h in HEADERS:
        h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
        named |= set(re.findall(r"#define (DD_\w+) ", h)) | set(re.findall(r"\b(DD_\w+) = ", h))
    assert consts == named and len(consts) >= 48
    assert L.ABI_VERSION == L.DD_ABI_VERSION == 6 and L.DD_DEV_VAE_TAIL == 64 and L.DD_DEV_EE_TAIL == 64
    assert L.DD_ERR_UNSUPPORTED == -6 and L.DD_DEV_NO_FRAG_X == 262144 and L.DD_PROF_SPLITK == 5
    assert len(L.SIGNATURES) == sum(len(re.findall(r"\bdd_\w+\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S))) for h in HEADERS) >= 108
    assert sum(len(s._fields_) for s in STRUCTS.values()) >= 238


# ---- the parser, one construct at a time ------------------------------------------------------------------------------------------
PRELUDE = "typedef struct dd_ctx dd_ctx;\ntypedef struct dd_s { int32_t n; } dd_s;\n"


def _parse(text, dev=False):
    return L.parse_header(PRELUDE + text, dev)


def test_parser_accepts_what_the_headers_use():
    _, types, _ = _parse("typedef struct dd_m { const float *a, *b_dev; int32_t B, C; uint64_t seed; dd_ctx* owner; const dd_s* s; } dd_m;")
    assert types["dd_m"]._fields_ == [("a", C.POINTER(C.c_float)), ("b_dev", C.c_void_p), ("B", C.c_int32), ("C", C.c_int32),
                                      ("seed", C.c_uint64), ("owner", C.c_void_p), ("s", C.POINTER(types["dd_s"]))]
    assert types["dd_ctx"] is None and issubclass(types["dd_s"], C.Structure)
    _, types, _ = _parse("typedef struct dd_m { const float *a, *b_dev; unsigned short* h; } dd_m;", dev=True)     # duodiff_dev.h: addresses only
    assert [t for _, t in types["dd_m"]._fields_] == [C.c_void_p] * 3
    _, _, sig = _parse("int dd_f(long long out3[3], int n[]);")                                 # an array parameter is a pointer
    assert sig == {"dd_f": (C.c_int, [C.c_void_p, C.c_void_p])}
    consts, _, _ = _parse("#define DD_A 32u\n#define DD_B 7\n#define NOT_OURS 3.5\n#define DD_GUARD_H_SEEN 1\n")
    assert consts == {"DD_A": 32, "DD_B": 7, "DD_GUARD_H_SEEN": 1}
    consts, _, _ = _parse("typedef enum dd_e { DD_OK = 0, DD_ERR_X = -1,\n DD_ERR_Y = -12 } dd_e;\nenum { DD_P = 0, DD_Q = 1 };")
    assert consts == {"DD_OK": 0, "DD_ERR_X": -1, "DD_ERR_Y": -12, "DD_P": 0, "DD_Q": 1}
    _, types, sig = _parse("int dd_f(const float* a, float const* b, float* const c, const dd_s* s, dd_s const* t, const char* name);")
    assert sig["dd_f"][1] == [C.c_void_p] * 3 + [C.POINTER(types["dd_s"])] * 2 + [C.c_char_p]
    _, _, sig = _parse("int dd_v(void);\nvoid dd_w(dd_ctx* ctx);\nconst char* dd_n(void);\nint64_t dd_c(const dd_ctx* c);\nlong long dd_l(dd_ctx** out);")
    assert sig == {"dd_v": (C.c_int, []), "dd_w": (None, [C.c_void_p]), "dd_n": (C.c_char_p, []), "dd_c": (C.c_int64, [C.c_void_p]),
                   "dd_l": (C.c_longlong, [C.c_void_p])}
    _, _, sig = _parse("int dd_t(int a, int32_t b, unsigned c, uint32_t d, int64_t e, uint64_t f, long long g, unsigned long long h,\n"
                       "         unsigned short i, float j, double k, size_t l, void* m, void** n);")
    assert sig["dd_t"][1] == [C.c_int, C.c_int32, C.c_uint, C.c_uint32, C.c_int64, C.c_uint64, C.c_longlong, C.c_ulonglong, C.c_ushort,
                              C.c_float, C.c_double, C.c_size_t, C.c_void_p, C.c_void_p]
    _, _, sig = _parse('/* int dd_hidden(int); */\n#ifdef __cplusplus\nextern "C" {\n#endif\nint dd_x(int a); // int dd_gone(int);\n'
                       "#ifdef __cplusplus\n}\n#endif\n")
    assert list(sig) == ["dd_x"]


@pytest.mark.parametrize("text, names", [
    ("int dd_f(dd_ctx* ctx, foo_t x);", "foo_t"),                                                    # an unknown type name
    ("typedef struct dd_m { int32_t n; bar_t* p; } dd_m;", "bar_t"),
    ("int dd_f(dd_ctx* ctx, dd_s by_value);", "dd_s by_value"),
    ("int dd_f(dd_ctx* ctx, void (*done)(int));", "(*done)"),                                         # a function pointer
    ("typedef struct dd_m { int (*cb)(int); } dd_m;", "(*cb)"),
    ("typedef struct dd_m { unsigned flags : 3; } dd_m;", "flags : 3"),                               # a bit-field
    ("typedef struct dd_m { struct { int a; } inner; } dd_m;", "inner"),                              # a nested struct
    ("typedef struct dd_m { int32_t n; union dd_u* u; } dd_m;", "dd_u"),
    ("typedef struct { int a; } dd_m;", "dd_m"),                                                      # an anonymous struct
    ("typedef struct dd_m { float rows[4]; } dd_m;", "rows[4]"),                                      # an array field
    ("#define DD_SCALE 0.18215\n", "DD_SCALE 0.18215"),                                               # a DD_ value that is no integer
    ('#define DD_NAME "duodiff"\n', "DD_NAME"),
    ("#define DD_MASK (1 << 4)\n", "DD_MASK"),
    ("#define DD_EMPTY\n", "DD_EMPTY"),
    ("enum { DD_A, DD_B };", "DD_A"),                                                                 # an enumerator without a value
    ("int dd_f(int);", "dd_f"),                                                                       # a parameter without a name
    ("int dd_f(int a)", "dd_f"),                                                                      # no terminating semicolon
])
def test_parser_refuses_everything_else(text, names):
    with pytest.raises(L.HeaderError) as e:
        _parse(text)
    assert names in str(e.value), str(e.value)


def test_missing_header_is_engine_unavailable(tmp_path, monkeypatch):
    monkeypatch.setattr(L, "INCLUDE", tmp_path)
    with pytest.raises(L.EngineUnavailable, match=re.escape(str(tmp_path / "duodiff.h"))):
        L._bind()


# ---- the longest prototypes, written out from the headers' text ---------------------------------------------------------------------
KIND = {"p": C.c_void_p, "i": C.c_int, "f": C.c_float}


def _kinds(spec):
    """'p i*7 f' -> [c_void_p, c_int x 7, c_float]"""
    out = []
    for tok in spec.split():
        k, _, n = tok.partition("*")
        out += [KIND[k]] * int(n or 1)
    return out


def test_longest_prototypes_position_by_position():
    tail = _kinds("p i*7 p*14 p*7 i p i p p")          # ctx | B .. poison | h_host .. wqkv | xres_host .. slab_host | slab_rows plan_out iters stream ms_out
    assert len(tail) == 34 and L.SIGNATURES["dd_dev_block_tail"] == (C.c_int, tail)
    assert L.SIGNATURES["dd_dev_block_tail_frag"] == (C.c_int, tail + _kinds("p*5")) and len(tail) + 5 == 39
    # ctx | precision M N K K1 | A A2 W bias | epilogue .. resid | ln | tok_l tok_e | xres_host out_host | ldo | h_host frag_host slab_host | num_cus iters | stream ms_out
    assert L.SIGNATURES["dd_dev_gemm"] == (C.c_int, _kinds("p i*5 p*4 i*6 p i*2 p*2 i p*3 i*2 p p")) and len(L.SIGNATURES["dd_dev_gemm"][1]) == 29
    # ctx | x m z h | thr | a b c d p q | use_hist | out | B C S | stream
    thr = _kinds("p p*4") + [C.POINTER(L.dd_x0_threshold)] + _kinds("f*6 i p i*3 p")
    assert len(thr) == 18 and L.SIGNATURES["dd_threshold_step"] == (C.c_int, thr)
    # ctx | B C S P D extras num_classes normalize generic | x_img w bias pos label_emb y t_vec | t_state | ln x_tok_host ln_frag_host | iters stream ms_out
    assert L.SIGNATURES["dd_dev_embed"] == (C.c_int, _kinds("p i*9 p*7 f p*3 i p p")) and len(L.SIGNATURES["dd_dev_embed"][1]) == 24
    # ctx vae | encode | in_dev out_dev | B hw | tap | stream; the tap record: ordinal | 6 host buffers | 5 capacities | 8 results | 4 sizes
    assert L.SIGNATURES["dd_dev_vae_trace"] == (C.c_int, _kinds("p p i p p i i") + [C.POINTER(L.dd_dev_vae_tap)] + _kinds("p"))
    assert [t for _, t in L.dd_dev_vae_tap._fields_] == _kinds("i p*6") + [C.c_longlong] * 5 + _kinds("i*8") + [C.c_longlong] * 4
    f = L.dd_dev_final_args._fields_
    assert len(f) == 60 and f[-1] == ("seed_out", C.c_ulonglong) and f[0] == ("B", C.c_int) and f[8] == ("dec", C.c_void_p)
    assert dict(f)["w_stride"] is C.c_longlong and dict(f)["guide_scale"] is C.c_float and dict(f)["h"] is C.c_void_p
    assert L.SIGNATURES["dd_dev_final"] == (C.c_int, [C.c_void_p, C.POINTER(L.dd_dev_final_args), C.c_void_p])
    # the public header's host row arrays stay typed, its device pointers and handles are addresses
    assert dict(L.dd_affine_sample_args._fields_)["noise"] == C.POINTER(C.c_int32) and dict(L.dd_affine_sample_args._fields_)["x_dev"] is C.c_void_p
    assert dict(L.dd_multistep_sample_args._fields_)["h_dev"] is C.c_void_p and dict(L.dd_sample_args._fields_)["first"] is C.c_void_p
    assert L.SIGNATURES["dd_model_set_param"] == (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int])
    assert L.SIGNATURES["dd_last_sample_timing"] == (C.c_int, [C.c_void_p, C.c_void_p]) and L.SIGNATURES["dd_build_id"] == (C.c_char_p, [])


def test_round_trip_through_the_built_library():
    lib = L.load()
    assert lib.dd_abi_version() == L.ABI_VERSION
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert re.fullmatch(r"[0-9a-f]{16}", lib.dd_build_id().decode())
