"""ctypes binding of libscint_hip.so (the C ABI in include/scint_hip.h).

There is no CPU fallback: if the library or a GPU is missing, every compute
entry point raises.  Loading the library itself needs only the HIP runtime, so
``symbols()`` works in a GPU-less container (the CPU test-suite checks that the
library exports everything the header declares).
"""
import collections
import ctypes
import operator
import os
import re
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_size_t, c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libscint_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "scint_hip.h")

SCINT_OK = 0
SCINT_E_ARG = 1
SCINT_E_NOCONV = 4
SCINT_E_EMPTY = 5
SCINT_E_NONFINITE = 6


class ScintHipError(RuntimeError):
    """A call into libscint_hip.so failed (message from scint_last_error)."""
    status = None      # the SCINT_E_* code, where a call returned one


class CsGeom(ctypes.Structure):
    """Mirror of scint_cs_geom."""
    _fields_ = [("ntau", c_int64), ("nfd", c_int64),
                ("tau0", c_double), ("dtau", c_double),
                ("fd0", c_double), ("dfd", c_double),
                ("tau_max", c_double), ("fd_max", c_double),
                ("tau1_step", c_double), ("fd1_step", c_double)]


class ThinGeom(ctypes.Structure):
    """Mirror of scint_thin_geom."""
    _fields_ = [("ntau", c_int64), ("nfd", c_int64),
                ("tau1", c_double), ("dtau", c_double),
                ("fd1", c_double), ("dfd", c_double)]


# ---- the binding is derived from include/scint_hip.h -------------------------------------------------------------------
_SCALARS = {"int32_t": c_int32, "int64_t": c_int64, "double": c_double, "size_t": c_size_t}
_HOST_POINTEES = dict(_SCALARS, char=ctypes.c_char, scint_cs_geom=CsGeom, scint_thin_geom=ThinGeom)
_DEVICE_POINTEES = ("scint_c128", "double", "float", "int32_t", "int64_t", "uint8_t", "void")
_STRUCTS = {"scint_cs_geom": CsGeom, "scint_thin_geom": ThinGeom}
# Entry points whose int32_t is a VALUE (a count, a mode), not a status: `call` hands it back instead of checking it.
_RETURNS_VALUE = frozenset(("scint_version", "scint_device_count", "scint_sweep_precision", "scint_sweep_workgroups"))

# kind: "scalar" | "host" | "device"; ctype: the argtype; pointee: the type name the header gives a pointer's target
Param = collections.namedtuple("Param", "name kind ctype pointee const")


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _symbols(text):
    return sorted(set(re.findall(r"\b(scint_[a-z0-9_]+)\s*\(", text)))


def _parse_param(decl, proto):
    m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*)?\s*(SCINT_HOST)?\s*(\w+)", decl.strip())
    if not m:
        raise ValueError(f"scint_hip.h: cannot read parameter `{decl.strip()}` of `{proto}`")
    const, typ, star, host, name = m.groups()
    if not star:
        if typ not in _SCALARS or host:
            raise ValueError(f"scint_hip.h: unknown type `{typ}` of parameter `{name}` of `{proto}`")
        return Param(name, "scalar", _SCALARS[typ], typ, True)
    if host:
        if typ not in _HOST_POINTEES:
            raise ValueError(f"scint_hip.h: unknown host pointee `{typ}` of parameter `{name}` of `{proto}`")
        return Param(name, "host", c_char_p if typ == "char" else POINTER(_HOST_POINTEES[typ]), typ, bool(const))
    if typ not in _DEVICE_POINTEES:
        raise ValueError(f"scint_hip.h: unknown device pointee `{typ}` of parameter `{name}` of `{proto}`")
    return Param(name, "device", c_void_p, typ, bool(const))


def parse_header(text):
    """(SCINT_ABI_VERSION, {entry point: [Param, ...]}) of a header text.  Raises ValueError for anything it cannot read: a
    prototype the strict pattern misses, an unknown type, a geometry struct that differs from its ctypes mirror."""
    text = _strip_comments(text)
    ver = re.search(r"^\s*#\s*define\s+SCINT_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    if not ver:
        raise ValueError("scint_hip.h: no `#define SCINT_ABI_VERSION <number>`")
    protos = {}
    for m in re.finditer(r"\bint32_t\s+(scint_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        proto = " ".join(m.group(0).split())
        args = m.group(2).strip()
        protos[m.group(1)] = [] if args == "void" else [_parse_param(d, proto) for d in args.split(",")]
    unread = sorted(set(_symbols(text)) - set(protos))
    if unread:
        raise ValueError(f"scint_hip.h: cannot read the prototype of {', '.join(unread)} "
                         "(expected `int32_t scint_name(type name, ...);`)")
    for m in re.finditer(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;", text):
        mirror = _STRUCTS.get(m.group(2))
        if mirror is None:
            continue
        want = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):      # `double tau0, dtau`
            typ, names = decl.split(None, 1)
            want += [(n.strip(), _SCALARS.get(typ)) for n in names.split(",")]
        if want != list(mirror._fields_) or ctypes.sizeof(mirror) != sum(ctypes.sizeof(t) for _, t in want):
            raise ValueError(f"scint_hip.h: {m.group(2)} has fields {[n for n, _ in want]} ({len(want)}), "
                             f"{mirror.__name__} mirrors {[n for n, _ in mirror._fields_]} ({len(mirror._fields_)})")
    return int(ver.group(1)), protos


with open(HEADER_PATH) as _fh:
    ABI_VERSION, _PARAMS = parse_header(_fh.read())       # ABI_VERSION: scint_version() of the library this binding describes
_SIGNATURES = {name: ([p.ctype for p in params], c_int32) for name, params in _PARAMS.items()}

_lib = None


def header_symbols():
    """Names of every function declared in include/scint_hip.h."""
    with open(HEADER_PATH) as fh:
        return _symbols(_strip_comments(fh.read()))


# ---- one checked way across the boundary -------------------------------------------------------------------------------
def _device_dtypes(torch):
    return {"scint_c128": (torch.complex128,), "double": (torch.float64,), "float": (torch.float32, torch.complex64),
            "int32_t": (torch.int32,), "int64_t": (torch.int64,), "uint8_t": (torch.uint8,), "void": None}


def _converter(fn_name, p, torch):
    """The function that checks one argument of `fn_name` against parameter `p` and turns it into what ctypes passes.  It only
    checks: an array or tensor of the wrong type, layout or residence is a TypeError, never a silent copy."""
    where = f"{fn_name}: parameter `{p.name}`"
    if p.kind == "scalar":
        return float if p.ctype is c_double else operator.index      # (a float for a size is a TypeError, not truncated)
    if p.kind == "device":
        dtypes = _device_dtypes(torch)[p.pointee]
        expect = f"a contiguous torch tensor of {p.pointee}" + (", an address" if dtypes is None else "") + " or None"

        def device(t):
            if t is None:
                return None
            if isinstance(t, torch.Tensor):
                if dtypes is not None and t.dtype not in dtypes:
                    raise TypeError(f"{where} is `{p.pointee}*` device memory: expected {expect}, got a tensor of {t.dtype}")
                if not t.is_contiguous():
                    raise TypeError(f"{where}: expected {expect}, got a non-contiguous tensor")
                return t.data_ptr()
            if dtypes is None and type(t) is int:
                return t
            raise TypeError(f"{where} is `{p.pointee}*` device memory: expected {expect}, got {type(t).__name__}")
        return device
    ctype = _HOST_POINTEES[p.pointee]
    dtype = np.dtype(ctype) if p.pointee in _SCALARS else None
    expect = (f"a C-contiguous{'' if p.const else ' writeable'} NumPy array of {dtype}, " if dtype is not None else "") + \
        f"a ctypes {ctype.__name__} (or an array of them) or None"

    def host(a):
        if a is None:
            return None
        if isinstance(a, np.ndarray):
            if dtype is None or a.dtype != dtype:
                raise TypeError(f"{where} is `{p.pointee}*` host memory: expected {expect}, got an array of {a.dtype}")
            if not a.flags.c_contiguous:
                raise TypeError(f"{where}: expected {expect}, got a non-contiguous array")
            if not (p.const or a.flags.writeable):
                raise TypeError(f"{where} is written by the call: expected {expect}, got a read-only array")
            return a.ctypes.data_as(p.ctype)
        if isinstance(a, ctype):
            return ctypes.byref(a)
        if isinstance(a, ctypes.Array) and a._type_ is ctype:
            return a
        raise TypeError(f"{where} is `{p.pointee}*` host memory: expected {expect}, got {type(a).__name__}")
    return host


def bind(lib):
    """Give every entry point of a loaded library (the product's, or the emulated one of the tests) the argument types the
    header declares and the converters `call` uses.  Returns `lib`.  AttributeError, as ctypes' own, if it lacks a symbol."""
    import torch
    missing = [name for name in _PARAMS if not hasattr(lib, name)]
    if missing:
        raise AttributeError(f"{getattr(lib, '_name', lib)} lacks {', '.join(missing)}, which include/scint_hip.h declares")
    lib._calls = {}
    for name, params in _PARAMS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = _SIGNATURES[name]
        lib._calls[name] = (fn, [_converter(name, p, torch) for p in params])
    return lib


def call(name, *args):
    """Call entry point `name`: every argument is checked against the header's parameter (scalar, host pointer, device
    pointer -- TypeError before the library is entered) and the status is checked (ScintHipError).  Returns None, or the
    value of the few entry points that return one (scint_version, scint_sweep_precision, ...)."""
    lib = load()
    try:
        fn, convs = lib._calls[name]
    except AttributeError:             # a library handle that was put in place without `bind` (tests may do that)
        fn, convs = bind(lib)._calls[name]
    if len(args) != len(convs):
        raise TypeError(f"{name} takes {len(convs)} arguments ({len(args)} given)")
    rc = fn(*[conv(a) for conv, a in zip(convs, args)])
    if name in _RETURNS_VALUE:
        return rc
    check(rc, name)


def load():
    """Load (once) and return the ctypes library.  Raises ScintHipError if the
    shared object has not been built (python -m scintools_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScintHipError(
            f"{LIB_PATH} is missing: build it with `python -m scintools_amd.build` "
            "(there is no CPU fallback)")
    # PyTorch-ROCm ships its own HIP runtime; it must be in the process BEFORE our library is
    # loaded so that both bind the same runtime (loading ours first leaves the process with two
    # runtimes and ours then sees no device).
    import torch  # noqa: F401
    # An entry point may be ADDED without a new ABI version (the version guards the argument lists of the existing ones): a stale
    # build that lacks one must say so here, not fail with an AttributeError in the middle of a call.
    try:
        lib = bind(ctypes.CDLL(LIB_PATH))
    except AttributeError as err:
        raise ScintHipError(f"{err}: it was built from older sources; rebuild it with `python -m scintools_amd.build`") from None
    # The header describes ONE version of the C ABI (an argument added in the middle of a list shifts every
    # pointer after it): a stale build must fail here, not corrupt memory in its first call.
    got = lib.scint_version()
    if got != ABI_VERSION:
        raise ScintHipError(f"{LIB_PATH} implements version {got} of the C ABI, this package binds version {ABI_VERSION}: "
                            "rebuild it with `python -m scintools_amd.build`")
    _lib = lib
    return lib


def last_error():
    buf = ctypes.create_string_buffer(1024)
    load().scint_last_error(buf, len(buf))
    return buf.value.decode(errors="replace")


def check(rc, what=""):
    if rc != SCINT_OK:
        err = ScintHipError(f"{what or 'libscint_hip call'} failed (status {rc}): {last_error()}")
        err.status = rc
        raise err


def require_gpu():
    """Fail loudly when no MI355X is visible -- the product never computes on the CPU."""
    lib = load()
    if lib.scint_device_count() < 1:
        raise ScintHipError("no HIP device visible: scintools_amd has no CPU fallback")
    return lib
