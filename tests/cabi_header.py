"""Reader of include/diffsep_hip.h and its comparison with the hand-written ctypes copy in diffsep_amd/_lib.py: the
prototypes against _lib._SIGS, the structs against the ctypes classes (names, classes, sizes and offsets), the integer
#defines against their Python twins.  Everything works on text and on ctypes types: no library is loaded."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "diffsep_hip.h")

# every struct that crosses the boundary and the ctypes class of _lib that mirrors it
STRUCTS = {"diffsep_model_config": "ModelConfig", "diffsep_sde_config": "SdeConfig", "diffsep_sampler_config": "SamplerConfig",
           "diffsep_sampler_ext": "SamplerExt", "diffsep_ode_config": "OdeConfig", "diffsep_ode_info": "OdeInfo",
           "diffsep_ode_ext": "OdeExt", "diffsep_loss_config": "LossConfig", "diffsep_prof_record": "ProfRecord"}

SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
           "char": C.c_char}
_SCALAR_NAME = {v: k for k, v in SCALARS.items()}


def read_header():
    with open(HEADER) as f:
        return f.read()


def _decl(text):
    """one declarator with its type, `const float* x` / `int64_t shape[4]` / `float* const* K` -> ((base, depth), name,
    array length or None); depth = the number of `*`"""
    text = re.sub(r"\bconst\b", " ", text)
    depth = text.count("*")
    words = text.replace("*", " ").split()
    base, name = " ".join(words[:-1]), words[-1]
    arr = re.fullmatch(r"(\w+)\[(\d+)\]", name)
    return (base, depth), (arr.group(1) if arr else name), (int(arr.group(2)) if arr else None)


def parse(text):
    """(prototypes, structs, constants) of the header text:
    prototypes {name: ((base, depth) of the result, [((base, depth), parameter name)])}, an array parameter counted as a pointer;
    structs {name: [(field, (base, depth), array length | None)]} in declaration order, `a, b` lists expanded;
    constants {"DIFFSEP_X": int} for every #define with an integer value."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    consts = {n: int(v, 0) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DIFFSEP_\w+)[ \t]+(-?(?:0x)?[0-9a-fA-F]+)[ \t]*$",
                                                  text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"', " ", text)
    structs = {}

    def take_struct(m):
        fields = []
        for decl in (d.strip() for d in m.group(2).split(";")):
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(",")]
            typ, name, arr = _decl(first)
            fields.append((name, typ, arr))
            for d in more:  # (the stars of `T* a, b` would bind to a alone; the header has no such list)
                _, name, arr = _decl("x " + d)
                fields.append((name, typ, arr))
        structs[m.group(3)] = fields
        return " "
    text = re.sub(r"typedef\s+struct\s*(\w+)?\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)
    protos = {}
    for stmt in text.replace("{", " ").replace("}", " ").split(";"):
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(diffsep_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if not m:
            continue
        res = _decl(m.group(1) + " _")[0]
        params = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                (base, depth), name, arr = _decl(p)
                params.append(((base, depth + (arr is not None)), name))
        protos[m.group(2)] = (res, params)
    return protos, structs, consts


def _c_name(typ):
    return typ[0] + "*" * typ[1]


def _py_name(t, struct_names):
    """what a ctypes type of _SIGS / of a struct field says in the header's words; "pointer" = any pointer"""
    if t is None:
        return "void"
    if t is C.c_void_p:
        return "pointer"
    if t is C.c_char_p:
        return "char*"
    if t in _SCALAR_NAME:
        return _SCALAR_NAME[t]
    if hasattr(t, "contents"):  # POINTER(X)
        return _py_name(t._type_, struct_names) + "*"
    return struct_names.get(t, t.__name__)


def _agree(py, typ):
    if py == "pointer":
        return typ[1] >= 1
    if py == "pointer*":
        return typ[1] == 2
    return py == _c_name(typ)


def field_ctype(typ, arr):
    """the ctypes type a struct field of the header lays out as"""
    t = C.c_void_p if typ[1] else SCALARS[typ[0]]
    return t * arr if arr is not None else t


def compare_prototypes(parsed, sigs, struct_classes):
    """Differences between the header's prototypes and sigs (_lib._SIGS) as a list of strings that each name the function and
    the argument position: presence on both sides, result type, argument count, each argument's class.  `pointer` in sigs
    agrees with any pointer, POINTER(X) only with a pointer to the struct X mirrors (struct_classes {C struct name: ctypes
    class}) or to the scalar X is."""
    protos = parsed[0]
    names = {cls: name for name, cls in struct_classes.items()}
    out = []
    for name in sorted(set(protos) | set(sigs)):
        if name not in sigs:
            out.append(f"{name}: declared in the header, missing from _SIGS")
            continue
        if name not in protos:
            out.append(f"{name}: in _SIGS, not declared in the header")
            continue
        (res, params), (pres, pargs) = protos[name], sigs[name]
        if _py_name(pres, names) != _c_name(res):
            out.append(f"{name}: returns {_c_name(res)} in the header, {_py_name(pres, names)} in _SIGS")
        if len(params) != len(pargs):
            out.append(f"{name}: {len(params)} arguments in the header, {len(pargs)} in _SIGS")
            continue
        for i, ((typ, pname), parg) in enumerate(zip(params, pargs)):
            if not _agree(_py_name(parg, names), typ):
                out.append(f"{name} argument {i} ({pname}): {_c_name(typ)} in the header, {_py_name(parg, names)} in _SIGS")
    return out


def compare_structs(parsed, struct_classes):
    """Differences between the header's structs and their ctypes classes, each naming the struct and the field: the set of
    structs, field names in order, each field's class, and its offset and size against the layout ctypes gives the header's
    own types."""
    structs = parsed[1]
    names = {cls: name for name, cls in struct_classes.items()}
    out = []
    for name in sorted(set(structs) | set(struct_classes)):
        if name not in struct_classes:
            out.append(f"{name}: struct of the header with no ctypes class listed")
            continue
        if name not in structs:
            out.append(f"{name}: struct not found in the header")
            continue
        cls, fields = struct_classes[name], structs[name]
        if [f[0] for f in cls._fields_] != [f[0] for f in fields]:
            out.append(f"{name}: fields {[f[0] for f in fields]} in the header, {[f[0] for f in cls._fields_]} in ctypes")
            continue
        want = type(name, (C.Structure,), {"_fields_": [(n, field_ctype(typ, arr)) for n, typ, arr in fields]})
        for (fname, typ, arr), (_, ptype) in zip(fields, cls._fields_):
            elem = ptype._type_ if arr is not None and hasattr(ptype, "_length_") else ptype
            if not _agree(_py_name(elem, names), typ):
                out.append(f"{name}.{fname}: {_c_name(typ)} in the header, {_py_name(elem, names)} in ctypes")
            a, b = getattr(want, fname), getattr(cls, fname)
            if (a.offset, a.size) != (b.offset, b.size):
                out.append(f"{name}.{fname}: offset {a.offset} size {a.size} in the header, offset {b.offset} size {b.size} in ctypes")
        if C.sizeof(want) != C.sizeof(cls):
            out.append(f"{name}: sizeof {C.sizeof(want)} in the header, {C.sizeof(cls)} in ctypes")
    return out


def compare(parsed, sigs, struct_classes):
    return compare_prototypes(parsed, sigs, struct_classes) + compare_structs(parsed, struct_classes)


def compare_constants(parsed, lib_module, conv_classes):
    """Differences between the header's DIFFSEP_<NAME> integers and their Python twins: _lib.<NAME>, _lib.GN_ROUTES[<name>] for
    DIFFSEP_GN_<NAME>, len(conv_classes) for DIFFSEP_NUM_KERNEL_CLASSES.  A constant without a twin is a difference."""
    out = []
    missing = object()
    for name, value in sorted(parsed[2].items()):
        short = name[len("DIFFSEP_"):]
        if short == "NUM_KERNEL_CLASSES":
            mine = len(conv_classes)
        elif short.startswith("GN_"):
            mine = lib_module.GN_ROUTES.get(short[3:].lower(), missing)
        else:
            mine = getattr(lib_module, short, missing)
        if mine is missing:
            out.append(f"{name} = {value} in the header has no Python twin")
        elif mine != value:
            out.append(f"{name}: {value} in the header, {mine} in Python")
    return out
