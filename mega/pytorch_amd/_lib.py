"""ctypes binding of libmega_hip.so, derived from include/mega_hip.h.

The header is the one declaration of the C ABI: the kernels' sources include it (the compiler checks every definition
against its prototype) and this module parses it into SIGNATURES, PARAMS and STRUCTS.  Nothing here is typed by hand, so a
new entry point needs its prototype in the header, its definition under csrc/ and a wrapper in ops.py.  The grammar the
parser accepts is stated in the header's "Boundary rules"; a declaration outside it raises, naming the line.

The product path has NO fallback: if the library or the header is missing or a call fails, this raises.
"""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libmega_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(HERE, "..", "..", "include", "mega_hip.h"))

c_int, c_float, c_void_p, c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
c_longlong = ctypes.c_longlong

_ERR = {1: "bad argument", 2: "kernel launch failure", 3: "workspace too small", 4: "kernel loop bound exceeded"}

_SCALARS = {"int": c_int, "float": c_float, "long long": c_longlong, "size_t": c_size_t}
_RETURNS = {"int": c_int, "size_t": c_size_t, "void": None, "const char*": ctypes.c_char_p}


def _declarator(decl):
    """`TYPE name` -> (name, ctype); any pointer is a c_void_p.  None outside the grammar."""
    m = re.match(r"^(.*?)\s*(\w+)$", decl.strip())
    if not m:
        return None
    if "*" in m.group(1):
        return m.group(2), c_void_p
    typ = _SCALARS.get(" ".join(m.group(1).split()))
    return None if typ is None else (m.group(2), typ)


def parse_header(text, path="mega_hip.h"):
    """The declarations of a header in the grammar of mega_hip.h's "Boundary rules" ->
    ({name: (restype, argtypes)}, {name: parameter names}, {typedef name: ctypes.Structure subclass})."""
    # comments become their own newlines, so that a position still tells its line
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    text = re.sub(r'^[ \t]*#[^\n]*|^extern "C" \{$|^\}$', "", text, flags=re.M)      # preprocessor lines, the extern "C" block
    signatures, params, structs = {}, {}, {}
    end = 0
    for st in re.finditer(r"((?:[^;{]|\{[^}]*\})*);", text):
        end = st.end()
        decl = " ".join(st.group(1).split())
        if not decl:
            continue

        def bad(why):
            return ValueError("%s:%d: %s -- outside the binding's grammar (see the header's Boundary rules): %r"
                              % (path, text.count("\n", 0, st.end(1) - len(st.group(1).lstrip())) + 1, why, decl))

        m = re.match(r"^typedef struct \{(.*)\} (mega_\w+)$", decl)
        if m:
            fields = []
            for field in filter(None, (f.strip() for f in m.group(1).split(";"))):
                names = [n.strip() for n in field.split(",")]
                first = _declarator(names[0])
                if first is None or not all(re.match(r"^\w+$", n) for n in names[1:]):
                    raise bad("field `%s`" % field)
                fields += [first] + [(n, first[1]) for n in names[1:]]
            structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {"_fields_": fields})
            continue
        m = re.match(r"^(.*?)\s*\b(mega_\w+)\s*\((.*)\)$", decl)
        if not m:
            raise bad("neither a prototype nor a typedef struct")
        ret = re.sub(r"\s*\*\s*", "*", m.group(1))
        if ret not in _RETURNS:
            raise bad("return type `%s`" % m.group(1))
        args = [] if m.group(3).strip() == "void" else [(p, _declarator(p)) for p in m.group(3).split(",")]
        for p, d in args:
            if d is None:
                raise bad("parameter `%s`" % p.strip())
        signatures[m.group(2)] = (_RETURNS[ret], [d[1] for _, d in args])
        params[m.group(2)] = tuple(d[0] for _, d in args)
    rest = text[end:].lstrip()
    if rest:
        raise ValueError("%s:%d: unterminated declaration: %r" % (path, text.count("\n", 0, len(text) - len(rest)) + 1,
                                                                   rest.strip()))
    return signatures, params, structs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(
            "include/mega_hip.h not found at %s -- the ctypes binding of libmega_hip.so is derived from it; "
            "mega.pytorch_amd runs from the repository tree (there is no hand-written signature table to fall back on)"
            % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return parse_header(f.read(), HEADER_PATH)


# name -> (restype, argtypes) / parameter names of every entry point; typedef name -> ctypes.Structure of every descriptor
SIGNATURES, PARAMS, STRUCTS = _read_header()

_lib = None


def load():
    """Load the library (once).  Raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libmega_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the MEGA hot path)" % LIB_PATH)
    # torch bundles its own libamdhip64.so.7; ours must resolve to THAT copy (one HIP runtime per process:
    # streams / device pointers are shared with torch).  Loading this library before torch would bind
    # /opt/rocm's copy instead and every launch would fail with hipErrorNoDevice.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        detail = ""
        if rc == 2 and _lib is not None:
            detail = ": " + _lib.mega_last_error_string().decode()
        raise RuntimeError("%s failed: %s (code %d)%s" % (what, _ERR.get(rc, "unknown"), rc, detail))
