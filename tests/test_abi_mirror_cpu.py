"""The Python binding's mirror of include/mwengine.h (miniworld_amd/engine.py), whole, without a GPU: every constant, every struct's
layout and every function's signature.  ctypes restates the public header by hand on purpose (tests/test_world_fields_cpu.py says why);
this is what keeps the two from drifting — a member added on one side only would otherwise be read as garbage without a word.  The
header is regular enough for `re`; the layouts come from the C++ compiler (tests/hostcheck/abi_layout.cpp)."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mwengine.h")

# the naming rule: the binding's constant is the header's name without the MW_ prefix, except for these
RENAMED = {"MW_FC_MAX_SLOTS": "MAX_FRAME_CACHE"}        # (miniworld_amd/csrc/mw_frame_plan.h: not in the public header, mirrored all the same)
# header constants the binding leaves out: it reports a status code as the number in an EngineError and names none
LEFT_OUT = {"MW_OK", "MW_E_INVALID", "MW_E_HIP", "MW_E_NOMEM", "MW_E_CAPACITY", "MW_E_DEVICE", "MW_E_OVERFLOW"}

STRUCTS = {"mw_range": "MwRange", "mw_config": "MwConfig", "mw_poly": "MwPoly", "mw_state_view": "MwStateView", "mw_prog_room": "MwProgRoom",
           "mw_prog_op": "MwProgOp", "mw_gen_program": "MwGenProgram", "mw_plan_trace": "MwPlanTrace", "mw_nav_params": "MwNavParams",
           "mw_ray_params": "MwRayParams"}
MEMBER_RENAMED = {("mw_range", "def"): "default"}       # (`def` is a Python keyword)


def uncommented(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_constants(text):
    """every integer #define MW_* and every MW_* enumerator: name -> value (a value may name an earlier constant)"""
    text = uncommented(text)
    found = [(m.group(1), m.group(2)) for m in re.finditer(r"^#define[ \t]+(MW_\w+)[ \t]+(\S+)[ \t]*$", text, re.M)]
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        items = [item.strip() for item in body.split(",") if item.strip()]
        assert all(re.fullmatch(r"MW_\w+\s*=\s*\S+", item) for item in items), body        # every enumerator was understood
        found += [tuple(re.split(r"\s*=\s*", item)) for item in items]
    out = {}
    for name, value in found:
        assert name not in out, name
        out[name] = out[value] if value in out else int(value, 0)
    return out


def header_structs(text):
    """struct name -> member names in order, for every `typedef struct ... { ... } name;` of the header"""
    out = {}
    for body, name in re.findall(r"typedef struct(?: \w+)? \{([^}]*)\} (\w+);", uncommented(text)):
        members = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            kind, rest = re.fullmatch(r"((?:const )?\w+)\s*(.*)", decl, re.S).groups()
            for declarator in rest.split(","):
                members.append(re.fullmatch(r"\s*\*?\s*(\w+)\s*(?:\[\w+\])*\s*", declarator).group(1))
        out[name] = members
    return out


def header_functions(text):
    """function name -> (return type, [parameter declarations]) for every prototype of the header"""
    out = {}
    for ret, name, params in re.findall(r"^([\w \*]+?)\b(mw_\w+)\(([^;{]*?)\);", uncommented(text), re.M | re.S):
        assert name not in out, name
        out[name] = (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
    return out


def c_class(decl):
    """pointer, i32 or i64: the class of a C parameter or return type"""
    if "*" in decl:
        return "pointer"
    kind = re.fullmatch(r"(?:const )?((?:unsigned )?(?:long long|\w+))(?: \w+)?", decl).group(1)
    return {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "unsigned long long": "i64"}[kind]


def ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    assert issubclass(t, C._SimpleCData) and t._type_ in "iIlLqQ", t
    return {4: "i32", 8: "i64"}[C.sizeof(t)]


@pytest.fixture(scope="module")
def header():
    return open(HEADER).read()


def test_every_constant_of_the_header_is_the_bindings(header):
    from miniworld_amd import engine
    consts = header_constants(header)
    frame_plan = open(os.path.join(ROOT, "miniworld_amd", "csrc", "mw_frame_plan.h")).read()
    consts["MW_FC_MAX_SLOTS"] = int(re.search(r"^#define MW_FC_MAX_SLOTS (\d+)$", frame_plan, re.M).group(1))
    assert len(consts) > 60 and consts["MW_ABI_VERSION"] == 4 and consts["MW_MAX_PLAN"] == consts["MW_MAX_REPEAT"] == 256
    assert LEFT_OUT <= set(consts) and set(RENAMED) <= set(consts)
    wrong = []
    for name, value in consts.items():
        if name in LEFT_OUT:
            continue
        mirror = RENAMED.get(name, name[len("MW_"):])
        if not hasattr(engine, mirror):
            wrong.append(f"{name}: the binding has no {mirror} (and the test's tables do not say why)")
        elif getattr(engine, mirror) != value or not isinstance(getattr(engine, mirror), int):
            wrong.append(f"{name} = {value}, engine.{mirror} = {getattr(engine, mirror)!r}")
    assert wrong == []


def compiled_layouts():
    """struct -> (sizeof, [(member, offset, size)]) as g++ lays the header out (tests/hostcheck/abi_layout.cpp)"""
    src, exe = os.path.join(HERE, "hostcheck", "abi_layout.cpp"), os.path.join(HERE, "hostcheck", "abi_layout")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in (src, HEADER)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-invalid-offsetof", src, "-o", exe])
    out = {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        words = line.split()
        if words[0] == "struct":
            out[words[1]] = (int(words[2]), [])
        else:
            out[words[1]][1].append((words[2], int(words[3]), int(words[4])))
    return out


def test_every_struct_is_laid_out_as_the_compiler_lays_it_out(header):
    from miniworld_amd import engine
    declared, compiled = header_structs(header), compiled_layouts()
    assert sorted(declared) == sorted(compiled) == sorted(STRUCTS)          # every struct of the header is compared
    for name, cls_name in STRUCTS.items():
        cls = getattr(engine, cls_name)
        size, members = compiled[name]
        assert [m for m, _, _ in members] == declared[name], name           # the host program leaves no member out
        mirror = [(MEMBER_RENAMED.get((name, m), m), off, sz) for m, off, sz in members]
        assert [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_] == mirror, name
        assert C.sizeof(cls) == size, name
    assert C.sizeof(engine.MwConfig) == 1504 and engine.POLY_DTYPE.itemsize == C.sizeof(engine.MwPoly)
    assert [engine.POLY_DTYPE.fields[n][1] for n, _ in engine.MwPoly._fields_] == [off for _, off, _ in compiled["mw_poly"][1]]


def test_every_function_is_declared_as_the_header_declares_it(header):
    from miniworld_amd import engine
    declared = header_functions(header)
    assert len(declared) > 60
    only_header = sorted(set(declared) - set(engine.SIGNATURES))
    only_binding = sorted(set(engine.SIGNATURES) - set(declared))
    assert only_header == [], f"declared in include/mwengine.h, without a signature in engine.SIGNATURES: {only_header}"
    assert only_binding == [], f"in engine.SIGNATURES, not declared in include/mwengine.h: {only_binding}"
    assert engine.EXPORTS == list(engine.SIGNATURES)
    returns = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}
    wrong = []
    for name, (ret, params) in declared.items():
        argtypes, restype = engine.SIGNATURES[name]
        if restype is not returns[ret]:
            wrong.append(f"{name}: returns {ret}, the binding says {restype}")
        want = [] if params == ["void"] else [c_class(p) for p in params]
        got = [ctypes_class(t) for t in argtypes]
        if want != got:
            wrong.append(f"{name}({', '.join(params)}): the binding passes {got}")
    assert wrong == []
    # a typed struct pointer is a pointer to the struct the header names there (arrays of mw_poly travel as plain addresses)
    for name, (_, params) in declared.items():
        for p, t in zip(params, engine.SIGNATURES[name][0]):
            if issubclass(t, C._Pointer) and issubclass(t._type_, C.Structure):
                m = re.match(r"(?:const )?(mw_\w+) \*", p)
                assert m and t._type_ is getattr(engine, STRUCTS[m.group(1)]), (name, p)


def test_load_library_applies_the_table():
    from miniworld_amd import engine
    engine.build_library()
    lib = engine.load_library()
    for name, (argtypes, restype) in engine.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
