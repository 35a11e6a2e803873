"""The C ABI of libgacq.so as ctypes, read from include/gacq.h: the header is the one definition, nothing here restates it.

    prototypes   {"gacq_search": (restype, [argtypes]), ...}     in the header's order
    signatures   {"gacq_search": ("int", ["gacq_sig*", "const float*", "size_t", ...]), ...}   the same as normalised C types
    structs      {"gacq_sigdesc": <ctypes.Structure subclass>, ...}     every `typedef struct NAME { ... } NAME;`
    constants    {"GACQ_ERR_BAD_ARG": -1, ...}                   every `#define GACQ_* <integer>`

Pure Python: no library, no numpy, no torch.  It reads the subset of C the header is written in -- scalars of SCALARS, pointers of
any depth and constness, array parameters and array members, opaque handles -- and raises CHeaderError with the declaration quoted
on anything else (an unknown type name, a function pointer, a bit-field, a union, a struct by value): it never guesses.

Pointers bind by one rule: `const char*` is c_char_p, every other pointer is c_void_p, as a parameter, a return value or a member.
c_void_p takes typed pointer objects, byref(), arrays, plain addresses and None, so the latency path passes addresses without a cast.
"""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gacq.h")

# every scalar type the header may spell, word for word (tests/test_native_cpu.py asks the compiler about each)
SCALARS = {
    "int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
    "signed char": ctypes.c_byte, "int8_t": ctypes.c_int8, "uint8_t": ctypes.c_uint8, "int16_t": ctypes.c_int16, "int32_t": ctypes.c_int32,
    "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
}
_TYPE_WORDS = {w for name in SCALARS for w in name.split()} | {"void", "char", "const", "signed", "short", "struct", "union", "enum"}


class CHeaderError(ValueError):
    """A declaration outside the subset of C this module reads"""


def ctype_of(ctype):
    """The ctypes type of a normalised C type ("int", "const void* const*"); None for void"""
    if ctype.endswith("*"):
        return ctypes.c_char_p if ctype == "const char*" else ctypes.c_void_p
    return None if ctype == "void" else SCALARS[ctype]


_TOKEN = re.compile(r"\w+|\S")
_STARS = re.compile(r"(\*( const)?( |$))*")


def _declarator(text, known, where, seen):
    """One `TYPE NAME` or `TYPE NAME[a][b]` -> (normalised C type, name, [a, b]); `known`: the struct and handle names so far;
    `seen`: what earlier calls of this parse returned (`gacq_ctx* ctx` stands in the header dozens of times)"""
    text = text.strip()
    if text not in seen:
        seen[text] = _read_declarator(text, known, where)
    return seen[text]


def _read_declarator(text, known, where):
    tokens, dims = _TOKEN.findall(text), []
    while len(tokens) > 3 and tokens[-1] == "]" and tokens[-2].isdigit() and tokens[-3] == "[":
        dims.insert(0, int(tokens[-2]))
        del tokens[-3:]
    if not tokens or not all(t == "*" or t[0].isalnum() or t[0] == "_" for t in tokens):
        raise CHeaderError("cannot read %r in: %s" % (text.strip(), where))
    name = tokens.pop()
    if name == "*" or name in _TYPE_WORDS or name in known or not tokens:
        raise CHeaderError("no name or no type in %r in: %s" % (text.strip(), where))
    # [const] WORDS then any number of `*` or `* const`
    words = tokens[tokens[0] == "const":]
    stars = next((i for i, t in enumerate(words) if t in ("*", "const")), len(words))
    base, stars = " ".join(words[:stars]), " ".join(words[stars:])
    if not _STARS.fullmatch(stars):
        raise CHeaderError("cannot read %r in: %s" % (text.strip(), where))
    if not (base in SCALARS or (stars and (base in ("void", "char") or base in known))):
        raise CHeaderError("unknown type %r (or a struct by value) in: %s" % (base, where))
    # the words as written, each * against the word before it: "const void* const*"
    return " ".join(tokens).replace(" *", "*"), name, dims


def parse(text):
    """(signatures, fields, constants) of a header's text; fields: {struct: [(name, C type, dims), ...]}"""
    before, *comments = text.split("/*")                           # comments out: what follows a /* up to the next */
    if comments and "*/" not in comments[-1]:
        raise CHeaderError("a comment without its end: /*%s" % comments[-1][:200])
    text = re.sub(r"//[^\n]*", " ", before + " ".join(part.partition("*/")[2] for part in comments))
    constants, defined, live, code = {}, set(), [], []
    for line in text.split("\n"):
        line = line.strip()
        if not line.startswith("#"):
            if all(live):
                code.append(line)
            continue
        m = re.fullmatch(r"#\s*(\w+)\s*(.*)", line)
        word, rest = (m.group(1), m.group(2).strip()) if m else ("", "")
        if word in ("ifdef", "ifndef") and re.fullmatch(r"\w+", rest):
            live.append((rest in defined) == (word == "ifdef"))
        elif word == "endif" and live:
            live.pop()
        elif word == "include":
            pass
        elif word == "define" and re.fullmatch(r"\w+(\s.*)?", rest) and not line.endswith("\\"):
            if all(live):
                name, _, value = rest.partition(" ")
                defined.add(name)
                v = re.fullmatch(r"\(\s*(-?\s*\d+)\s*\)|(-?\s*\d+)|(0[xX][0-9a-fA-F]+)", value.strip())
                if v:
                    constants[name] = int((v.group(1) or v.group(2) or v.group(3)).replace(" ", ""), 0)
                elif value.strip():
                    raise CHeaderError("not an integer constant: %s" % line)
        else:
            raise CHeaderError("cannot read the preprocessor line: %s" % line)
    if live:
        raise CHeaderError("#ifdef / #ifndef without #endif")
    constants = {k: v for k, v in constants.items() if k.startswith("GACQ_")}

    signatures, fields, known, seen = {}, {}, set(), {}
    body = " ".join(" ".join(code).split())
    # statements end at a ; outside braces
    statements, depth, start = [], 0, 0
    for m in re.finditer(r"[{};]", body):
        depth += {"{": 1, "}": -1, ";": 0}[m.group()]
        if m.group() == ";" and depth == 0:
            statements.append(body[start:m.start()].strip())
            start = m.end()
    if depth or body[start:].strip():
        raise CHeaderError("text after the last declaration: %s" % body[start:].strip()[:200])
    for st in statements:
        m = re.fullmatch(r"typedef struct (\w+) (\w+)", st)
        if m and m.group(1) == m.group(2):                         # an opaque handle
            known.add(m.group(1))
            continue
        m = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", st)
        if m and m.group(1) == m.group(3) and m.group(1) not in fields:
            name, members = m.group(1), []
            if "{" in m.group(2) or ":" in m.group(2) or not m.group(2).rstrip().endswith(";"):
                raise CHeaderError("a nested struct, a union, a bit-field or an unfinished member in: %s" % st)
            for decl in m.group(2).split(";")[:-1]:
                first, *more = decl.split(",")
                ctype, fname, dims = _declarator(first, known, st, seen)
                members.append((fname, ctype, dims))
                for other in more:                                 # `double a, b[2]`: the type of the first, never a pointer
                    if "*" in decl:
                        raise CHeaderError("several pointer members in one declaration: %s; in: %s" % (decl.strip(), st))
                    _, fname, dims = _declarator(ctype + " " + other, known, st, seen)
                    members.append((fname, ctype, dims))
            if len({f for f, _, _ in members}) != len(members):
                raise CHeaderError("a member name twice in: %s" % st)
            fields[name] = members
            known.add(name)
            continue
        head, paren, inside = st.partition("(")                    # RETURN-TYPE NAME ( PARAMETERS )
        if paren and inside.endswith(")") and "(" not in inside and ")" not in inside[:-1] and not st.startswith("typedef"):
            if len(head.split()) == 2 and head.split()[0] == "void":
                ret, name = head.split()
            else:
                ret, name, dims = _declarator(head, known, st, seen)
                if dims:
                    raise CHeaderError("cannot read: %s" % st)
            if not name.startswith("gacq_") or name in signatures:
                raise CHeaderError("not a gacq_ function, or declared twice: %s" % st)
            params = []
            if inside[:-1].strip() != "void":
                for p in inside[:-1].split(","):
                    ctype, _, dims = _declarator(p, known, st, seen)
                    params.append(ctype + "*" if dims else ctype)  # an array parameter is a pointer to its elements
                    if len(dims) > 1:
                        raise CHeaderError("an array parameter of several dimensions in: %s" % st)
            signatures[name] = (ret, params)
            continue
        raise CHeaderError("not a prototype, a struct or a handle of the subset this reads: %s" % st)
    return signatures, fields, constants


def _struct(name, members):
    cfields = []
    for fname, ctype, dims in members:
        t = ctype_of(ctype)
        for d in reversed(dims):                                   # T name[a][b] is (T * b) * a
            t = t * d
        cfields.append((fname, t))
    return type(name, (ctypes.Structure,), {"_fields_": cfields, "__doc__": "%s of include/gacq.h" % name})


def load(text):
    """(prototypes, signatures, structs, constants) of a header's text"""
    signatures, fields, constants = parse(text)
    prototypes = {name: (ctype_of(ret), [ctype_of(p) for p in params]) for name, (ret, params) in signatures.items()}
    return prototypes, signatures, {name: _struct(name, members) for name, members in fields.items()}, constants


if not os.path.exists(HEADER):
    raise ImportError("the C header %s is missing: the Python binding is derived from it (it sits beside the package, in include/)" % HEADER)
with open(HEADER, encoding="utf-8") as _f:
    prototypes, signatures, structs, constants = load(_f.read())
