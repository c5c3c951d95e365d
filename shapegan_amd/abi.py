"""Reader of the C ABI header: include/shapegan_hip.h is the only statement of the ABI, and everything else is derived from it.

lib.py builds its ctypes table (`name -> (restype, argtypes)`) from `DECLARATIONS`, build.py writes from them the `sg_<name>_cpu`
prototypes the compiler holds the C++ twin to, and the Python constants that mirror a `#define SG_*` read it through `defines()`.
Standard library only: the build imports this module without torch.  A missing header raises a RuntimeError when this module is
imported.  A declaration the reader cannot classify raises and names itself; no type ever falls back to a default.
"""
import collections
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(_HERE, "..", "include", "shapegan_hip.h")

Decl = collections.namedtuple("Decl", "name ret params")       # params: [(type text, parameter name)]

SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t, "hipStream_t": ctypes.c_void_p}
_POINTEES = (set(SCALARS) - {"hipStream_t"}) | {"void", "char", "unsigned char", "unsigned", "unsigned long long", "uint8_t", "int64_t", "sg_comm"}


def _read(path):
    if not os.path.exists(path):
        raise RuntimeError("the header %s is missing — the ctypes table, the twin's prototypes and the SG_* constants of the "
                           "Python side are read from the C headers" % path)
    with open(path) as f:
        return f.read()


def _strip(text, preprocessor):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M) if preprocessor else text


@functools.lru_cache(maxsize=None)
def _classify(text):
    """The ctypes class of a type's text (None for `void`); KeyError for anything the header does not use today."""
    words = text.replace("*", " * ").split()
    base = " ".join(w for w in words if w not in ("const", "*"))
    if words == ["void"]:
        return None
    if "*" not in words:
        return SCALARS[base]
    if base not in _POINTEES:
        raise KeyError(base)
    return ctypes.c_char_p if words == ["const", "char", "*"] else ctypes.c_void_p


def _ctype(text, where, returned=False):
    try:
        ctype = _classify(text)
    except KeyError:
        ctype = None
    if ctype is None and not (returned and text.split() == ["void"]):
        raise ValueError("shapegan_amd.abi: cannot classify the type '%s' in the declaration of %s" % (text.strip(), where))
    return ctype


@functools.lru_cache(maxsize=None)
def _normal(text):
    return re.sub(r"\s*\*", "*", " ".join(text.split()))


_PARAM = re.compile(r"^(.*[\s\*])([A-Za-z_]\w*)$", flags=re.S)
_NAME = re.compile(r"\bsg_\w+\s*\(")


def declarations(path):
    """Every `sg_*` prototype of the header at `path`: Decl(name, return type text, [(type text, parameter name)])."""
    text = _strip(_read(path), preprocessor=True)
    out = []
    for statement in text.split(";"):
        found = _NAME.search(statement)
        if not found:
            continue
        name = found.group(0).rstrip("( \t\n")
        ret = re.split(r'[{}"]', statement[:found.start()])[-1]        # what is left of an `extern "C" {` or a closing brace
        m = re.fullmatch(r"([^()]*)\)\s*", statement[found.end():])
        if not m:
            raise ValueError("shapegan_amd.abi: cannot read the declaration of %s" % name)
        _ctype(ret, name, returned=True)
        params = []
        if m.group(1).strip() not in ("", "void"):
            for arg in m.group(1).split(","):
                p = _PARAM.match(arg.strip())
                if not p:
                    raise ValueError("shapegan_amd.abi: cannot read the parameter '%s' of %s" % (arg.strip(), name))
                _ctype(p.group(1), name)
                params.append((_normal(p.group(1)), p.group(2)))
        out.append(Decl(name, _normal(ret), params))
    return out


def ctypes_signature(decl):
    """(restype, argtypes) of a declaration: scalars through SCALARS, `const char*` as c_char_p, every other pointer as c_void_p."""
    restype = _ctype(decl.ret, decl.name, returned=True)
    return restype, [_ctype(t, decl.name) for t, _ in decl.params]


def defines(path):
    """{name: value} of the `#define SG_<NAME> <integer literal>` macros of a header; other macro bodies are skipped."""
    text = _strip(_read(path), preprocessor=False)
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SG_\w+)[ \t]+(0[xX][0-9a-fA-F]+|[1-9]\d*|0)[uUlL]*[ \t]*$", text, flags=re.M)
    return {name: int(value, 0) for name, value in found}


def core_defines(header):
    """defines() of one of csrc/*_core.h, the arithmetic the HIP kernels share with the twin."""
    return defines(os.path.join(_HERE, "csrc", header))


def is_comm(name):
    """The RCCL gradient exchange lives in libshapegan_comm.so; every other entry point in libshapegan_hip.so."""
    return name.startswith(("sg_comm_", "sg_allreduce_"))


def twin_prototypes(decls):
    """The text of a header that declares `sg_<name>_cpu` for every entry point that has a twin, with the parameter list of
    include/shapegan_hip.h: compiled in front of csrc_cpu/shapegan_cpu.cpp, a twin that disagrees is a conflicting declaration."""
    lines = ["/* generated by shapegan_amd/build.py from include/shapegan_hip.h — do not edit */", "#include <stddef.h>", "#include <stdint.h>"]
    for d in decls:
        if d.name not in NO_TWIN and not is_comm(d.name):
            # the twin spells its unused stream parameter void*
            params = ", ".join("%s %s" % ("void*" if t == "hipStream_t" else t, n) for t, n in d.params)
            lines.append('extern "C" %s %s_cpu(%s);' % (d.ret, d.name, params or "void"))
    return "\n".join(lines) + "\n"


DECLARATIONS = declarations(HEADER)
DEFINES = defines(HEADER)
ABI_VERSION = DEFINES["SG_ABI_VERSION"]

# Entry points WITHOUT a twin: size queries and layout helpers are host code of libshapegan_hip.so (callable without a GPU; the
# twin keeps its opaque buffers within those sizes), the *_impl variants force a particular HIP kernel (tests / tuning).
NO_TWIN = {d.name for d in DECLARATIONS if not is_comm(d.name) and (d.name.endswith("_workspace_bytes") or d.name.endswith("_workspace_bytes_for") or d.name.endswith("_impl"))} | {
    "sg_sdfgen_acts_floats", "sg_sdfgen_packed_norm_offset", "sg_sdfgen_bwd_blocks", "sg_pointnet_packed_floats",
    "sg_abi_version", "sg_last_error", "sg_sdfnet_packed_floats", "sg_sdfnet_acts_floats", "sg_sdfnet_bwd_blocks", "sg_sdfnet_bwd_tile_start", "sg_sdf_batch_sort_max_shapes",
    "sg_conv3d_k4s2p1_wgrad_act_eligible", "sg_convT3d_k4s2p1_to1_pre_eligible", "sg_conv3d_k4s2p1_wgrad_dy_image",
    "sg_conv3d_k4s2p1_image_layout", "sg_gemm_plan", "sg_gemm_nt_plan"}
