"""ctypes binding of libjoeys2t_hip.so (the C ABI declared in include/joeys2t_hip.h).

There is no fallback: if the shared library is missing or a call is rejected, we raise.

The header is the only place a signature or a struct layout is written down: it is parsed at import, GemmDesc / AttnDesc are built
from its two structs and lib() sets restype / argtypes of every function it declares, so call sites pass plain Python values and a
value of the wrong kind (a float for an int64_t) is refused before the call.
"""
import ctypes as C
import os
import re
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("JS2T_LIB", PKG_DIR / "libjoeys2t_hip.so"))  # JS2T_LIB: instrumented builds of tools/
HEADER_PATH = PKG_DIR.parent / "include" / "joeys2t_hip.h"

F32, BF16 = 0, 1
ACT_CODES = {None: 0, "none": 0, "relu": 1, "gelu": 2, "swish": 3, "tanh": 4, "hardswish": 5}


class Js2tError(RuntimeError):
    pass


_CTYPES = {
    "int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
    "float": C.c_float, "double": C.c_double, "js2t_stream": C.c_void_p, "js2t_ctx": C.c_void_p,
}


def _ctype(spelling: str, decl: str, ret: bool = False):
    """the ctypes type of one C type spelling of the header; `decl` names the declaration in the error"""
    t = " ".join(spelling.replace("*", " * ").split())
    if "*" in t:
        return C.c_char_p if ret and t == "const char *" else C.c_void_p
    t = re.sub(r"\bconst\b", "", t).strip()
    if ret and t == "void":
        return None
    if t not in _CTYPES:
        raise Js2tError(f"{HEADER_PATH.name}: no ctypes type for '{spelling.strip()}' in '{' '.join(decl.split())}'")
    return _CTYPES[t]


def parse_header(text: str):
    """(structs, functions) of the public header: {struct name: [(field, ctype)]} and {function name: (restype, [argtypes])}."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", text):
        fields = structs[name] = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            base, head = re.fullmatch(r"(.*?)((?:\*\s*)*\w+)", first, flags=re.S).groups()
            for declarator in (head, *more):
                fields.append((declarator.replace("*", "").strip(), _ctype(base + "*" * declarator.count("*"), decl)))
    functions = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(js2t_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        decl = f"{ret} {name}({params})"
        params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)\w+", a.strip(), flags=re.S).group(1) for a in params.split(",")]
        functions[name] = (_ctype(ret, decl, ret=True), [_ctype(a, decl) for a in params])
    missed = set(re.findall(r"\b(js2t_[a-z0-9_]+)\s*\(", text)) - set(functions)
    if missed:
        raise Js2tError(f"{HEADER_PATH.name}: could not parse the declaration of {sorted(missed)}")
    return structs, functions


if not HEADER_PATH.exists():
    raise Js2tError(f"{HEADER_PATH} is missing: the Python binding reads every struct and signature from it")
STRUCTS, FUNCTIONS = parse_header(HEADER_PATH.read_text())


class GemmDesc(C.Structure):
    """js2t_gemm_desc (include/joeys2t_hip.h)."""
    _fields_ = STRUCTS["js2t_gemm_desc"]


class AttnDesc(C.Structure):
    """js2t_attn_desc (include/joeys2t_hip.h)."""
    _fields_ = STRUCTS["js2t_attn_desc"]


def declared_symbols():
    """Names of every function declared in the public header."""
    return sorted(FUNCTIONS)


_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the library was not built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise Js2tError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
            )
        # torch first: its wheel carries its own libamdhip64, and a process that has loaded /opt/rocm's copy through this library
        # BEFORE torch ends up with two HIP runtimes - the kernels' one then reports "no ROCm-capable device" (seen with
        # __graft_entry__.build() followed by smoke() in one process).  Loaded after torch, the library binds to torch's runtime:
        # one runtime, one set of streams and allocations.
        import torch  # noqa: F401
        handle = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in FUNCTIONS.items():  # every call converts and checks its arguments by the header's types
            fn = getattr(handle, name, None)
            if fn is None:
                raise Js2tError(f"{LIB_PATH} does not export {name}, which {HEADER_PATH.name} declares: rebuild the library")
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
        if "JS2T_P192" in os.environ:  # kernel-selection override for A/B measurements (see js2t_gemm_p192_mode)
            _lib.js2t_gemm_p192_mode(int(os.environ["JS2T_P192"]))
        if "JS2T_WG256" in os.environ:  # 0 / 1 / -1: the 256x128 kernel of the grouped weight gradients (js2t_gemm_wg256_mode)
            _lib.js2t_gemm_wg256_mode(int(os.environ["JS2T_WG256"]))
        if "JS2T_PANEL" in os.environ:  # 0 / 1 / -1: the panel-resident kernel (js2t_gemm_panel_mode)
            _lib.js2t_gemm_panel_mode(int(os.environ["JS2T_PANEL"]))
        if "JS2T_P192_RING" in os.environ:  # 2 = two blocks per CU with a two-slot ring (js2t_gemm_p192_ring)
            _lib.js2t_gemm_p192_ring(int(os.environ["JS2T_P192_RING"]))
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().js2t_last_error().decode("utf-8", "replace")
        raise Js2tError(f"libjoeys2t_hip: {what} failed (rc={rc}): {msg}")


CTX_KEYS = {"deterministic": 0, "gemm_p192_mode": 1, "gemm_p192_ring": 2, "gemm_wg256_mode": 3, "gemm_panel_mode": 4}


class Context:
    """A js2t_ctx (include/joeys2t_hip.h): the settings one caller's launches run with - deterministic mode, kernel-selection rules -
    bound to the calling thread for the length of a `with` block (the previous binding comes back at its end; blocks nest).

        ctx = Context(deterministic=True)
        with ctx:
            ...  # every library call made by this thread in here sees deterministic = 1

    Autograd's backward runs the library's kernels on worker threads unless told otherwise: TrainStep runs its backward passes under
    torch.autograd.set_multithreading_enabled(False), i.e. on the thread that holds the binding."""

    def __init__(self, **settings):
        self._h = lib().js2t_ctx_create()
        if not self._h:
            raise Js2tError("js2t_ctx_create failed")
        self._prev = []
        for k, v in settings.items():
            self.set(k, v)

    def set(self, key: str, value) -> None:
        check(lib().js2t_ctx_set(self._h, CTX_KEYS[key], int(value)), "js2t_ctx_set")

    def get(self, key: str) -> int:
        return lib().js2t_ctx_get(self._h, CTX_KEYS[key])

    def __enter__(self):
        self._prev.append(lib().js2t_ctx_bind(self._h))
        return self

    def __exit__(self, *exc):
        lib().js2t_ctx_bind(self._prev.pop())
        return False

    def __del__(self):
        try:
            if self._h and _lib is not None:
                _lib.js2t_ctx_destroy(self._h)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
        self._h = None


def effective(key: str) -> int:
    """the value of a context key the calling thread's next launch would see (process-wide test override > bound context > default)"""
    return lib().js2t_ctx_effective(CTX_KEYS[key])
