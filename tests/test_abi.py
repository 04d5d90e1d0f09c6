"""The ctypes mirror (_lib.py, _lib_tiled.py, _lib_resample.py, _lib_imgproc.py) against the C headers it restates by hand
(include/sr_hip.h, sr_tiled.h, sr_resample.h, sr_imgproc.h).  No GPU and no library needed: only the headers, the host C compiler and the Python tables.

* structs: a generated C program prints sizeof of every struct, offsetof + size of every member (the members of sr_op's union
  as ``u.ln.x`` and so on), the enumerators and the integer macros; these are compared with ctypes.sizeof, Field.offset / .size
  and the Python constants.  Every header struct must have a mirror and every mirror field a header member of the same name.
* functions: the prototypes are parsed and compared with the SYMBOLS tables: the same names both ways, the same arity, and per
  argument / return value the same class among pointer, int32, int64, float, double.  Each side library's header (SIDE) is also
  read the plain way, every `sr_name(` outside a comment: that set, the parsed prototypes and the table must be one set of the
  recorded size.
* the checker itself is run over mutated header text and mutated tables: each mutation must be reported."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from stable_renderer_amd import _lib as L
from stable_renderer_amd import _lib_imgproc as LI
from stable_renderer_amd import _lib_resample as LR
from stable_renderer_amd import _lib_tiled as LT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("sr_hip.h", "sr_tiled.h", "sr_resample.h", "sr_imgproc.h")
TABLES = {"sr_hip.h": L.SYMBOLS, "sr_tiled.h": LT.SYMBOLS, "sr_resample.h": LR.SYMBOLS, "sr_imgproc.h": LI.SYMBOLS}
SIDE = {"sr_tiled.h": 6, "sr_resample.h": 5, "sr_imgproc.h": 9}              # header -> number of exported functions
MIRRORS = {"sr_igemm_args": L.IgemmArgs, "sr_groupnorm_args": L.GroupNormArgs, "sr_attention_args": L.AttentionArgs, "sr_op": L.Op,
           "sr_draw": L.Draw, "sr_gbuffer": L.GBuffer}


def read_headers():
    out = {}
    for h in HEADERS:
        with open(os.path.join(INCLUDE, h)) as f:
            out[h] = f.read()
    return out


# ---- a small parser of the headers' C --------------------------------------------------------------------------------------

def strip(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return text


def macros(text):
    """integer #defines -> {name: value}"""
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$",
                                                                strip(text), flags=re.M)}


def tokens(text):
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", strip(text), flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    return re.findall(r"[A-Za-z_]\w*|-?\d+|[{}()\[\];,*=]", text)


class Parsed:
    def __init__(self):
        self.structs = {}        # typedef name -> [(member name, type tokens | nested member list, array length | None)]
        self.enums = {}          # enumerator -> value
        self.protos = {}         # function name -> (return type tokens, [argument type tokens])
        self.opaque = set()


def _block(tok, i):
    """tok[i] == '{' -> (tokens inside the matching braces, index after the closing brace)"""
    assert tok[i] == "{"
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(tok[j], 0)
        j += 1
    return tok[i + 1:j - 1], j


def _members(tok):
    """the member declarations of a struct / union body"""
    out, i = [], 0
    while i < len(tok):
        if tok[i] in ("struct", "union") and tok[i + 1] == "{":
            kind = tok[i]
            body, j = _block(tok, i + 1)
            assert tok[j + 1] == ";", "an anonymous struct / union declares one member"
            out.append((tok[j], (kind, _members(body)), None))
            i = j + 2
            continue
        j = tok.index(";", i)
        decl = tok[i:j]
        i = j + 1
        # `type a, b, c`: the type is everything before the first declarator; a `*` belongs to the declarator it precedes, but
        # these headers write `const float* x` with one declarator per pointer declaration
        parts, cur = [], []
        for t in decl:
            if t == ",":
                parts.append(cur)
                cur = []
            else:
                cur.append(t)
        parts.append(cur)
        first = parts[0]
        arr = None
        if first[-1] == "]":
            arr, first = int(first[-2]), first[:-3]
        base, name = first[:-1], first[-1]
        assert base, decl
        out.append((name, base, arr))
        for extra in parts[1:]:
            assert "*" not in base, f"several declarators after a pointer type: {decl}"
            arr = None
            if extra[-1] == "]":
                arr, extra = int(extra[-2]), extra[:-3]
            assert len(extra) == 1, decl
            out.append((extra[0], base, arr))
    return out


def parse(text):
    tok, P, i = tokens(text), Parsed(), 0
    while i < len(tok):
        if tok[i] == "}":                                          # the closing brace of extern "C"
            i += 1
        elif tok[i] == "typedef" and tok[i + 1] == "struct" and tok[i + 2] == "{":
            body, j = _block(tok, i + 2)
            P.structs[tok[j]] = _members(body)
            assert tok[j + 1] == ";"
            i = j + 2
        elif tok[i] == "typedef" and tok[i + 1] == "struct":      # typedef struct tag name;
            P.opaque.add(tok[i + 3])
            i = tok.index(";", i) + 1
        elif (tok[i] == "typedef" and tok[i + 1] == "enum") or tok[i] == "enum":
            k = tok.index("{", i)
            body, j = _block(tok, k)
            val = -1
            for item in " ".join(body).split(","):
                item = item.split()
                if not item:
                    continue
                val = int(item[2]) if len(item) == 3 and item[1] == "=" else val + 1
                P.enums[item[0]] = val
            i = tok.index(";", j - 1) + 1
        else:                                                      # a prototype: ret name ( args ) ;
            j = tok.index(";", i)
            decl = tok[i:j]
            i = j + 1
            k = decl.index("(")
            assert decl[-1] == ")", decl
            name, ret = decl[k - 1], decl[:k - 1]
            args, cur = [], []
            for t in decl[k + 1:-1]:
                if t == ",":
                    args.append(cur)
                    cur = []
                else:
                    cur.append(t)
            if cur:
                args.append(cur)
            if args == [["void"]]:
                args = []
            assert name not in P.protos, name
            P.protos[name] = (ret, [_arg_type(a) for a in args])
    return P


def _arg_type(a):
    """the type tokens of one parameter: the trailing identifier is its name (these headers name every parameter)"""
    a = [t for t in a if t != "const"]
    if len(a) > 1 and a[-1] != "*" and re.match(r"[A-Za-z_]", a[-1]):
        a = a[:-1]
    return a


INT32 = {"int", "int32_t", "uint32_t", "unsigned", "sr_status", "sr_dtype", "sr_op_kind"}


def c_class(t, where=""):
    t = [x for x in t if x != "const"]
    if "*" in t:
        return "ptr"
    assert len(t) == 1, (where, t)
    if t[0] in INT32:
        return "i32"
    return {"int64_t": "i64", "uint64_t": "i64", "float": "f32", "double": "f64", "void": "void"}[t[0]]


def ctypes_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "ptr"
    return {C.c_int32: "i32", C.c_uint32: "i32", C.c_int64: "i64", C.c_uint64: "i64", C.c_float: "f32", C.c_double: "f64"}[t]


# ---- structs ----------------------------------------------------------------------------------------------------------------

def header_paths(P, name):
    """every member path of struct `name`, nested members and members of known struct types expanded"""
    def walk(members, prefix):
        for mname, typ, arr in members:
            path = prefix + mname
            yield path
            if isinstance(typ, tuple):
                yield from walk(typ[1], path + ".")
            elif len(typ) == 1 and typ[0] in P.structs:
                yield from walk(P.structs[typ[0]], path + ".")
    return list(walk(P.structs[name], ""))


def measure(headers, tmp_path, tag="t"):
    """compile and run a program that prints the layout the host C compiler gives the headers' structs, their enumerators and
    integer macros -> (Parsed of all headers, {"struct": size}, {"struct.path": (offset, size)}, {enumerator / macro: value})"""
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    d = tmp_path / tag
    (d / "include").mkdir(parents=True)
    allp = Parsed()
    lines = ["#include <stdio.h>", "#include <stddef.h>"]
    mac = {}
    for h, text in headers.items():
        (d / "include" / h).write_text(text)
        lines.append(f'#include "{h}"')
        P = parse(text)
        allp.structs.update(P.structs)
        allp.enums.update(P.enums)
        allp.protos.update(P.protos)
        mac.update(macros(text))
    lines.append("int main(void) {")
    for s in allp.structs:
        lines.append(f'  printf("S {s} %zu\\n", sizeof({s}));')
        for path in header_paths(allp, s):
            lines.append(f'  printf("M {s}.{path} %zu %zu\\n", offsetof({s}, {path}), sizeof((({s}*)0)->{path}));')
    for e in allp.enums:
        lines.append(f'  printf("E {e} %lld\\n", (long long)({e}));')
    for m in mac:
        lines.append(f'  printf("E {m} %lld\\n", (long long)({m}));')
    lines += ["  return 0;", "}"]
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    exe = str(d / "layout")
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", str(d / "include"), str(d / "layout.c"), "-o", exe], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    sizes, members, values = {}, {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "S":
            sizes[f[1]] = int(f[2])
        elif f[0] == "M":
            members[f[1]] = (int(f[2]), int(f[3]))
        else:
            values[f[1]] = int(f[2])
    return allp, sizes, members, values


def mirror_paths(cls):
    """{path: (offset, size)} of a ctypes Structure, nested Structures / Unions expanded"""
    out = {}

    def walk(c, prefix, base):
        for fname, ftype in c._fields_:
            fd = getattr(c, fname)
            out[prefix + fname] = (base + fd.offset, fd.size)
            if isinstance(ftype, type) and issubclass(ftype, (C.Structure, C.Union)):
                walk(ftype, prefix + fname + ".", base + fd.offset)
    walk(cls, "", 0)
    return out


def struct_problems(sizes, members, mirrors):
    probs = []
    for s in sizes:
        if s not in mirrors:
            probs.append(f"struct {s}: no ctypes mirror")
    for s, cls in mirrors.items():
        if s not in sizes:
            probs.append(f"mirror {cls.__name__}: no struct {s} in the headers")
            continue
        if C.sizeof(cls) != sizes[s]:
            probs.append(f"{s}: sizeof {sizes[s]} in C, {C.sizeof(cls)} in ctypes")
        want = {k[len(s) + 1:]: v for k, v in members.items() if k.startswith(s + ".")}
        have = mirror_paths(cls)
        for path in want:
            if path not in have:
                probs.append(f"{s}.{path}: member missing in the mirror")
            elif have[path] != want[path]:
                probs.append(f"{s}.{path}: (offset, size) {want[path]} in C, {have[path]} in ctypes")
        for path in have:
            if path not in want:
                probs.append(f"{s}.{path}: mirror field without a header member")
    return probs


# ---- functions --------------------------------------------------------------------------------------------------------------

def function_problems(protos, table, what):
    probs = []
    for name in protos:
        if name not in table:
            probs.append(f"{what}: {name} is declared in the header and missing from the table")
    for name, (res, args) in table.items():
        if name not in protos:
            probs.append(f"{what}: {name} is in the table and not declared in the header")
            continue
        ret, hargs = protos[name]
        if c_class(ret, name) != ctypes_class(res):
            probs.append(f"{what}: {name} returns {c_class(ret, name)} in C, {ctypes_class(res)} in the table")
        if len(hargs) != len(args):
            probs.append(f"{what}: {name} takes {len(hargs)} arguments in C, {len(args)} in the table")
            continue
        for i, (h, t) in enumerate(zip(hargs, args)):
            if c_class(h, name) != ctypes_class(t):
                probs.append(f"{what}: {name} argument {i} is {c_class(h, name)} in C, {ctypes_class(t)} in the table")
    return probs


def all_problems(headers, tables, mirrors, tmp_path, tag):
    allp, sizes, members, _ = measure(headers, tmp_path, tag)
    probs = struct_problems(sizes, members, mirrors)
    for h, text in headers.items():
        probs += function_problems(parse(text).protos, tables[h], h)
    return probs


# ---- the tests --------------------------------------------------------------------------------------------------------------

def test_parser_sees_the_whole_header():
    P = parse(read_headers()["sr_hip.h"])
    assert set(P.structs) == set(MIRRORS) and P.opaque == {"sr_model"}
    assert len(P.protos) == len(L.SYMBOLS) >= 61
    assert P.protos["sr_last_error"] == (["const", "char", "*"], []) and c_class(P.protos["sr_last_error"][0]) == "ptr"
    assert [c_class(a) for a in P.protos["sr_silu"][1]] == ["ptr", "ptr", "i64", "i32", "ptr"]
    assert [c_class(a) for a in P.protos["sr_igemm_group"][1]] == ["ptr", "i32", "ptr"]
    paths = header_paths(P, "sr_op")
    assert {"kind", "lane", "u", "u.igemm.tile_order", "u.gn.eps", "u.attn.scale", "u.ln.x", "u.ln.n_frames", "u.cvt.scale", "u.temb.dtype",
            "u.ew.cols", "u.gather.err_flag", "u.add.dtype"} <= set(paths)
    assert {m for m in paths if m.count(".") == 1} == {"u." + n for n, _ in L._OpU._fields_}       # the nine union members
    assert "MV" in header_paths(P, "sr_draw") and "MV_IT" in header_paths(P, "sr_draw") and "P" in header_paths(P, "sr_draw")


def test_struct_layouts_match_the_headers(tmp_path):
    allp, sizes, members, values = measure(read_headers(), tmp_path)
    assert set(sizes) == set(MIRRORS)
    assert len(members) > 200
    assert struct_problems(sizes, members, MIRRORS) == []
    assert members["sr_draw.MV"][1] == 64 and members["sr_op.u"][1] == C.sizeof(L._OpU)


def test_constants_match_the_headers(tmp_path):
    from stable_renderer_amd import ops, resample, tiled
    _, _, _, v = measure(read_headers(), tmp_path)
    assert (v["SR_OK"], v["SR_ERR_INVALID"], v["SR_ERR_LAUNCH"], v["SR_ERR_UNSUPPORTED"]) == (0, -1, -2, -3)
    assert (v["SR_TILED_OK"], v["SR_TILED_ERR_INVALID"], v["SR_TILED_ERR_LAUNCH"]) == (0, -1, -2)
    assert (v["SR_RESAMPLE_OK"], v["SR_RESAMPLE_ERR_INVALID"], v["SR_RESAMPLE_ERR_LAUNCH"]) == (0, -1, -2)
    assert (v["SR_F16"], v["SR_F32"]) == (L.SR_F16, L.SR_F32) == (v["SR_TILED_F16"], v["SR_TILED_F32"])
    kinds = {k[len("SR_OP_"):]: val for k, val in v.items() if k.startswith("SR_OP_")}
    mine = {k[len("OP_"):]: val for k, val in vars(L).items() if k.startswith("OP_")}
    assert kinds == mine and len(kinds) == 15
    assert resample.MODES == {"nearest-exact": v["SR_RESAMPLE_NEAREST_EXACT"], "nearest": v["SR_RESAMPLE_NEAREST"],
                              "bilinear": v["SR_RESAMPLE_BILINEAR"], "bicubic": v["SR_RESAMPLE_BICUBIC"], "area": v["SR_RESAMPLE_AREA"]}
    assert v["SR_IGEMM_GROUP_MAX"] == ops.GROUP_MAX and v["SR_IGEMM_SPLIT_COUNTERS"] == ops.SPLIT_COUNTERS
    assert v["SR_TILE_FEATHER_MAX"] == tiled.FEATHER_MAX


def test_function_tables_match_the_prototypes():
    headers = read_headers()
    probs = []
    for h in HEADERS:
        probs += function_problems(parse(headers[h]).protos, TABLES[h], h)
    assert probs == []


@pytest.mark.parametrize("header", sorted(SIDE))
def test_side_header_declares_exactly_its_table(header):
    """declared == bound, both ways, comments stripped; the library-specific halves (the symbols resolve, bad arguments are refused
    with their texts) are in test_tiled_ref.py, test_resample_ref.py and test_imgproc_ref.py"""
    text = read_headers()[header]
    declared = set(re.findall(r"\b(sr_[a-z0-9_]+)\s*\(", strip(text)))
    protos = parse(text).protos
    assert declared == set(TABLES[header]) == set(protos) and len(declared) == SIDE[header]
    assert function_problems(protos, TABLES[header], header) == []
    assert parse(text).structs == {}                            # no structs cross these ABIs


def _sub(text, old, new):
    assert text.count(old) == 1, (old, text.count(old))
    return text.replace(old, new)


def test_the_checker_reports_every_mutation(tmp_path):
    """one member inserted, one int32_t widened, one argument dropped, one prototype removed, one table entry given an extra
    argument -- and, on the table side, one int64 declared as int32, one entry dropped, one mirror field dropped"""
    headers = read_headers()
    hip = headers["sr_hip.h"]
    assert all_problems(headers, TABLES, MIRRORS, tmp_path, "clean") == []

    def with_hip(text):
        return dict(headers, **{"sr_hip.h": text})

    # one member inserted: everything after it shifts
    probs = all_problems(with_hip(_sub(hip, "int32_t B, Bk, Tq, Tk, heads, d, ldt, dtype;", "int32_t B, Bk, extra, Tq, Tk, heads, d, ldt, dtype;")),
                         TABLES, MIRRORS, tmp_path, "insert")
    assert any("sr_attention_args.extra: member missing" in q for q in probs) and any("sr_attention_args.Tq: (offset" in q for q in probs)
    assert any("sr_op.u.attn.scale" in q for q in probs)
    # one int32_t widened inside the union's anonymous struct
    probs = all_problems(with_hip(_sub(hip, "int64_t n; int32_t dtype; int32_t rows, cols; } ew;", "int64_t n; int64_t dtype; int32_t rows, cols; } ew;")),
                         TABLES, MIRRORS, tmp_path, "widen")
    assert any("sr_op.u.ew.dtype: (offset, size) (32, 8) in C, (32, 4)" in q for q in probs) and any("sr_op.u.ew.rows" in q for q in probs)
    # ... and in a prototype
    probs = all_problems(with_hip(_sub(hip, "int sr_silu(const void* x, void* y, int64_t n, int32_t dtype, void* stream);",
                                       "int sr_silu(const void* x, void* y, int32_t n, int32_t dtype, void* stream);")), TABLES, MIRRORS, tmp_path, "widen2")
    assert probs == ["sr_hip.h: sr_silu argument 2 is i32 in C, i64 in the table"]
    # one argument dropped
    probs = all_problems(with_hip(_sub(hip, "int sr_axpby(float* y, const float* x, int64_t n, float a, float b, void* stream);",
                                       "int sr_axpby(float* y, const float* x, int64_t n, float a, void* stream);")), TABLES, MIRRORS, tmp_path, "drop")
    assert probs == ["sr_hip.h: sr_axpby takes 5 arguments in C, 6 in the table"]
    # one prototype removed
    probs = all_problems(with_hip(_sub(hip, "int sr_graph_destroy(void* graph_exec);", "")), TABLES, MIRRORS, tmp_path, "remove")
    assert probs == ["sr_hip.h: sr_graph_destroy is in the table and not declared in the header"]
    # a whole struct without a mirror
    probs = all_problems(with_hip(_sub(hip, "int sr_graph_destroy(void* graph_exec);",
                                       "int sr_graph_destroy(void* graph_exec);\ntypedef struct { int32_t a; } sr_new_args;")), TABLES, MIRRORS, tmp_path, "new")
    assert probs == ["struct sr_new_args: no ctypes mirror"]
    # the other headers are checked too
    probs = all_problems(dict(headers, **{"sr_tiled.h": _sub(headers["sr_tiled.h"], "int32_t th, int32_t tw,\n                   void* stream);",
                                                                 "int32_t th, int64_t tw,\n                   void* stream);")}), TABLES, MIRRORS, tmp_path, "tiled")
    assert probs == ["sr_tiled.h: sr_tile_gather argument 8 is i64 in C, i32 in the table"]

    # the table side
    def with_table(name, entry):
        t = dict(L.SYMBOLS)
        if entry is None:
            del t[name]
        else:
            t[name] = entry
        return dict(TABLES, **{"sr_hip.h": t})
    res, args = L.SYMBOLS["sr_euler_step"]
    probs = all_problems(headers, with_table("sr_euler_step", (res, args + [C.c_void_p])), MIRRORS, tmp_path, "t_extra")
    assert probs == ["sr_hip.h: sr_euler_step takes 5 arguments in C, 6 in the table"]
    probs = all_problems(headers, with_table("sr_euler_step", (res, [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p])), MIRRORS, tmp_path, "t_i32")
    assert probs == ["sr_hip.h: sr_euler_step argument 2 is i64 in C, i32 in the table"]
    probs = all_problems(headers, with_table("sr_euler_step", (res, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p])), MIRRORS, tmp_path, "t_f64")
    assert probs == ["sr_hip.h: sr_euler_step argument 3 is f32 in C, f64 in the table"]
    probs = all_problems(headers, with_table("sr_euler_step", None), MIRRORS, tmp_path, "t_gone")
    assert probs == ["sr_hip.h: sr_euler_step is declared in the header and missing from the table"]
    probs = all_problems(headers, with_table("sr_groupnorm_scratch_floats", (C.c_int32, [C.c_int32, C.c_int32])), MIRRORS, tmp_path, "t_ret")
    assert probs == ["sr_hip.h: sr_groupnorm_scratch_floats returns i64 in C, i32 in the table"]

    class ShortGBuffer(C.Structure):
        _fields_ = [f for f in L.GBuffer._fields_ if f[0] != "canny"]
    probs = all_problems(headers, TABLES, dict(MIRRORS, sr_gbuffer=ShortGBuffer), tmp_path, "m_short")
    assert any("sr_gbuffer.canny: member missing in the mirror" in q for q in probs) and any("sr_gbuffer.zbuf: (offset" in q for q in probs)

    class LongGBuffer(C.Structure):
        _fields_ = list(L.GBuffer._fields_) + [("spare", C.c_int32)]
    probs = all_problems(headers, TABLES, dict(MIRRORS, sr_gbuffer=LongGBuffer), tmp_path, "m_long")
    assert any("sr_gbuffer.spare: mirror field without a header member" in q for q in probs)
