"""CPU tier: shapegan_amd/abi.py, the reader that derives the ctypes table, the twin's prototypes and the Python copies of the
SG_* constants from the C headers.  The reader is tried on small headers written here, and on the real header against rows and
numbers written here by hand, independently of it."""
import os
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_void_p

import pytest

import shapegan_amd.lib as L
from shapegan_amd import abi

_P, _I, _L, _F, _Z, _D = c_void_p, c_int, c_long, c_float, c_size_t, c_double


def _declare(tmp_path, text):
    path = tmp_path / "header.h"
    path.write_text(text)
    return abi.declarations(str(path))


def test_every_type_form(tmp_path):
    decls = _declare(tmp_path, """
        #ifndef X
        #define X
        typedef struct ihipStream_t* hipStream_t;
        typedef struct sg_comm sg_comm;
        extern "C" {
        int sg_scalars(int a, long b, long long c, float d, double e, size_t f, hipStream_t stream);
        size_t sg_pointers(const float* const* a, long long* const* b, sg_comm** c, unsigned char* d, const int64_t* e, void* f,
                           const void *g, float * h, unsigned long long* i, const char* name);
        const char* sg_text(void);
        void sg_nothing();
        long long sg_wide(const char* path);
        }
        #endif
    """)
    assert [d.name for d in decls] == ["sg_scalars", "sg_pointers", "sg_text", "sg_nothing", "sg_wide"]
    assert decls[0].params == [("int", "a"), ("long", "b"), ("long long", "c"), ("float", "d"), ("double", "e"), ("size_t", "f"),
                               ("hipStream_t", "stream")]
    assert decls[1].params[:3] == [("const float* const*", "a"), ("long long* const*", "b"), ("sg_comm**", "c")]
    assert decls[1].params[6:8] == [("const void*", "g"), ("float*", "h")]
    assert (decls[2].ret, decls[2].params, decls[3].ret, decls[3].params) == ("const char*", [], "void", [])
    assert abi.ctypes_signature(decls[0]) == (c_int, [c_int, c_long, c_longlong, c_float, c_double, c_size_t, c_void_p])
    assert abi.ctypes_signature(decls[1]) == (c_size_t, [c_void_p] * 9 + [c_char_p])
    assert abi.ctypes_signature(decls[2]) == (c_char_p, [])
    assert abi.ctypes_signature(decls[3]) == (None, [])
    assert abi.ctypes_signature(decls[4]) == (c_longlong, [c_char_p])


def test_multi_line_prototypes_and_comments(tmp_path):
    decls = _declare(tmp_path, """
        /* int sg_x(int a); inside a block comment
         * that goes on: int sg_x(int); */
        // int sg_x(int a);
        int sg_three_lines(const float* x,   /* a comment between parameters */
                           long n,           // and another
                           hipStream_t stream);
        #define SG_CALL(x) sg_x(x)
    """)
    assert decls == [abi.Decl("sg_three_lines", "int", [("const float*", "x"), ("long", "n"), ("hipStream_t", "stream")])]


@pytest.mark.parametrize("text, named", [
    ("int sg_bad(unsigned n);", "sg_bad"),                # an unknown scalar
    ("int sg_bad(short n);", "sg_bad"),
    ("sg_handle sg_bad(int n);", "sg_bad"),               # an unknown return type
    ("int sg_bad(const widget* w);", "sg_bad"),           # a pointer to something the header never names
    ("int sg_bad(int (*callback)(int));", "sg_bad"),      # a form the reader does not know
])
def test_unknown_types_raise_and_name_the_declaration(tmp_path, text, named):
    with pytest.raises(ValueError, match=named):
        _declare(tmp_path, text)


def test_missing_header_says_so(tmp_path):
    with pytest.raises(RuntimeError, match="missing"):
        abi.declarations(str(tmp_path / "none.h"))
    with pytest.raises(RuntimeError, match="missing"):
        abi.defines(str(tmp_path / "none.h"))


def test_defines(tmp_path):
    path = tmp_path / "header.h"
    path.write_text("""
        #define SG_PLAIN 12
        #define SG_COMMENTED 3616 /* 14 * 256 + 32 */
        #define SG_SLASHED 256      // terms per tile
        #  define SG_HEX 0x10
        #define SG_LONG 9223372036854775807LL
        #define SG_SHIFT (1L << 20)
        #define SG_FLOAT 1e-3
        #define SG_NEGATIVE (-1)
        #define SG_CALL(x) f(x)
        #define OTHER 5
        // #define SG_IN_COMMENT 1
    """)
    assert abi.defines(str(path)) == {"SG_PLAIN": 12, "SG_COMMENTED": 3616, "SG_SLASHED": 256, "SG_HEX": 16,
                                      "SG_LONG": 9223372036854775807}


# rows of the real header, transcribed by hand from include/shapegan_hip.h
ROWS = {
    "sg_abi_version": (c_int, []),
    "sg_last_error": (c_char_p, []),
    "sg_gemm": (c_int, [_P, _L, _L, _P, _L, _L, _P, _L, _L, _P, _P, _I, _I, _I, _I, _I, _F, _P, _Z, _P]),
    "sg_gemm_workspace_bytes": (_Z, [_I, _I]),
    "sg_gemm_plan": (c_int, [_P, _L, _L, _P, _L, _L, _L, _L, _I, _I, _I, _I, _P, _Z, _P]),
    "sg_gemm_nt_plan": (c_int, [_I, _I, _I, _L, _P]),
    "sg_loss_meansq_fwd": (c_int, [_P, _P, _L, _I, _D, _P, _P, _Z, _P]),
    "sg_conv3d_k4s2p1_image_layout": (c_longlong, [_I, _P, _Z]),
    "sg_sdfnet_bwd_blocks": (c_long, [_L]),
    "sg_adam_step_dev_multi": (c_int, [_I] + [_P] * 14),
    "sg_emd_match": (c_int, [_P, _P, _L, _L, _D, _P, _P, _P, _P, _P]),
    "sg_simplify_bounds": (c_int, [_P, _P, _L, _L, _P, _P, _P]),
    "sg_comm_bind": (c_int, [c_char_p]),
    "sg_allreduce_init": (c_int, [_P, _I, _I, _P, _Z, _I]),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_real_header_rows(name):
    table = L.COMM_SIGNATURES if name.startswith(("sg_comm_", "sg_allreduce_")) else L.SIGNATURES
    restype, argtypes = table[name]
    assert restype is ROWS[name][0]
    assert len(argtypes) == len(ROWS[name][1]) and all(a is b for a, b in zip(argtypes, ROWS[name][1])), argtypes


def test_tables_cover_the_header():
    assert len(L.SIGNATURES) + len(L.COMM_SIGNATURES) == len(abi.DECLARATIONS) == len({d.name for d in abi.DECLARATIONS})
    assert sorted(L.COMM_SIGNATURES) == sorted(n for n in (d.name for d in abi.DECLARATIONS) if n.startswith(("sg_comm_", "sg_allreduce_")))
    assert not set(L.SIGNATURES) & set(L.COMM_SIGNATURES)
    assert abi.NO_TWIN <= set(L.SIGNATURES) and L.NO_TWIN is abi.NO_TWIN
    assert abi.ABI_VERSION == 8
    assert (L.ACT_NONE, L.ACT_LEAKY, L.ACT_RELU, L.ACT_TANH, L.ACT_SIGMOID) == (0, 1, 2, 3, 4)


def test_constants_read_from_the_headers():
    from shapegan_amd import evaluation, ops, optim, prepare, simplify, topology
    assert (ops._PART_ROW, ops._GEN_PART_ROW) == (3616, 7200)
    assert (ops._LATENT_TILE, ops._LATENT_ROW, ops._PROJECT_TILE) == (32, 513, 32)
    assert ops.TSNE_MAX_POINTS == 65536
    assert (prepare.MAX_SCANS, prepare.CHUNK) == (64, 256)
    assert evaluation._EMD_MAX_POINTS == 2048
    assert topology.TILE == 256
    assert simplify.MAX_CELLS == 16384
    assert ops.PROJECT_RULES == {"newton": 0, "unit": 1}
    assert optim._ADAM_DEV_WORDS == 544
    for value in (ops._PART_ROW, ops.TSNE_MAX_POINTS, topology.TILE, optim._ADAM_DEV_WORDS):
        assert type(value) is int


TWIN = """
extern "C" int sg_simplify_bounds_cpu(const float* vertices, const int64_t* vert_offsets, %s S, long V, float* lo, float* hi, void*) {
    return vertices && vert_offsets && lo && hi ? (int)(S + V) : 0;
}
"""


def test_twin_prototypes_hold_the_twin_to_the_header(tmp_path):
    """The generated prototypes in front of a twin's definition: the header's parameter list compiles, one `long` turned into
    `int` is a conflicting declaration."""
    protos = tmp_path / "twin_prototypes.h"
    text = abi.twin_prototypes(abi.DECLARATIONS)
    protos.write_text(text)
    twins = [d.name for d in abi.DECLARATIONS if d.name in L.SIGNATURES and d.name not in abi.NO_TWIN]
    assert text.count('extern "C"') == len(twins) and "hipStream_t" not in text
    assert 'extern "C" int sg_simplify_bounds_cpu(' in text and "sg_abi_version" not in text and "sg_allreduce" not in text
    results = {}
    for third in ("long", "int"):
        src = tmp_path / ("twin_%s.cpp" % third)
        src.write_text(TWIN % third)
        results[third] = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-fsyntax-only", "-include", str(protos), str(src)],
                                        capture_output=True, text=True)
    assert results["long"].returncode == 0, results["long"].stderr
    assert results["int"].returncode != 0 and "conflicting declaration of C function" in results["int"].stderr, results["int"].stderr
