"""Reader of include/spnet_hip.h: the C prototypes as ctypes signatures.  Pure Python (no torch, no library), so an
external binder can use it as spnet_amd/_lib.py does.  Not a C parser: it knows the forms the header uses and raises
on anything else, because a prototype skipped or misread here would hand a kernel a wrong size or pointer."""
import re
from ctypes import c_float, c_int, c_long, c_uint, c_void_p

_RET = {"int": c_int, "long": c_long}     # int: launch status (checked by the binding), long: raw query / predicate
_BY_VALUE = {"int": c_int, "long": c_long, "float": c_float, "unsigned": c_uint, "unsigned int": c_uint}
_PROTO = re.compile(r"(\w+) (spnet_\w+) ?\(([^()]*)\)")
_WRAPPER = re.compile(r'extern\s+"C"\s*\{|\}')


def _argtype(param, stmt):
    if "*" in param and "[" not in param:
        return c_void_p
    words = [w for w in param.split() if w != "const"]
    ctype = _BY_VALUE.get(" ".join(words[:-1]))         # the last word is the parameter's name
    if ctype is None or words[-1] in _BY_VALUE or not words[-1].isidentifier():
        raise ValueError("spnet_hip.h: unsupported parameter %r in: %s" % (param, stmt))
    return ctype


def parse_header(text):
    """{name: (restype, [argtypes])} of every prototype in the header text, in header order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    sigs = {}
    for stmt in _WRAPPER.sub(" ", text).split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _PROTO.fullmatch(stmt)
        if m is None or m.group(1) not in _RET or m.group(2) in sigs:
            raise ValueError("spnet_hip.h: not a prototype `int|long spnet_<name>(<params>)`: %s" % stmt)
        sigs[m.group(2)] = (_RET[m.group(1)], [_argtype(p, stmt) for p in m.group(3).split(",")])
    return sigs
