"""include/rlt_hip.h as ctypes: its integer #defines, its prototypes and its struct bodies.

Not a C parser: the header is plain C in one regular style, and whatever falls outside that style raises instead of being skipped."""
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_void_p

SCALARS = {"int": c_int, "size_t": c_size_t, "float": c_float, "double": c_double,
           "uint32_t": c_uint32, "int32_t": c_int32, "int64_t": c_int64}
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(rlt_\w+)\s*\(([^()]*)\)\s*;")
_STRUCT = re.compile(r"(?:typedef\s+)?struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w*)\s*;")


def _fields(decl, defines, where):
    """`const float *a, *b[2]` | `float gain[RLT_N]` | `const float* const* x` | `int n` -> [(name, ctype), ...]: a pointer of any
    kind is a c_void_p, `[n]` makes an array of n."""
    base, rest = re.fullmatch(r"((?:(?:const|struct)\s+)*\w+)(.*)", decl.strip(), re.S).groups()
    out = []
    for d in rest.split(","):
        m = re.search(r"(\w+)\s*(?:\[\s*(\w+)\s*\])?$", d.strip())
        if m and "*" in d:
            t = c_void_p
        elif m and d.strip() == m.group(0) and base.split()[-1] in SCALARS:
            t = SCALARS[base.split()[-1]]
        else:
            raise RuntimeError(f"{where}: no ctypes for `{' '.join(decl.split())}`")
        name, dim = m.groups()
        if dim and dim not in defines and not dim.isdigit():
            raise RuntimeError(f"{where}: `{dim}` in `{' '.join(decl.split())}` is neither an integer nor a define")
        out.append((name, t * (defines[dim] if dim in defines else int(dim)) if dim else t))
    return out


def parse(text):
    """-> (defines {RLT_NAME: int}, prototypes {rlt_name: (restype, [argtypes])} in header order, structs {name: [(field, ctype)]})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines, prototypes, structs = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(RLT_\w+)(.*)$", text, re.M):
        if value.strip():                                   # the include guard has none
            try:
                defines[name] = int(value.strip(" \t()"), 0)
            except ValueError:
                raise RuntimeError(f"#define {name}: `{value.strip()}` is not an integer") from None
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    for tag, body, alias in _STRUCT.findall(text):
        structs[alias or tag] = [f for decl in body.split(";") if decl.strip() for f in _fields(decl, defines, "struct " + (alias or tag))]
    text = _STRUCT.sub("", text)
    for ret, name, params in _PROTOTYPE.findall(text):
        ret = "".join(re.sub(r"\bconst\b", "", ret).split())
        if ret != "char*" and ret not in SCALARS:
            raise RuntimeError(f"{name}: no ctypes for the return type `{ret}`")
        args = []
        for p in params.split(",") if params.strip() != "void" else ():
            (_, t), = _fields(p, defines, name)
            args.append(c_void_p if "[" in p else t)          # an array parameter is a pointer
        prototypes[name] = (c_char_p if ret == "char*" else SCALARS[ret], args)
    left = re.search(r"\brlt_\w+\s*\(", _PROTOTYPE.sub("", text))
    if left:
        raise RuntimeError(f"`{left.group(0)}...` is not a prototype that rlt_hip/header.py reads")
    return defines, prototypes, structs


def read(path):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes binding of librlt_hip.so is derived from it")
    with open(path) as f:
        return parse(f.read())
