"""validation/include/ntm/abi.h is the one declaration of the shipping C ABI; the
ctypes tables of ops/_lib.py (SIGNATURES, XGMI_SIGNATURES) are its Python view. The
.hip files include the header, so the compiler holds the definitions to it; this test
holds the Python tables to it, in both directions, name by name and argument by
argument. No GPU and no built library: the header is parsed with a small regular
expression, the tables are read as data."""
import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "validation" / "include" / "ntm" / "abi.h"
SRC = ROOT / "validation" / "src"

# Exported for C / C++ callers only - not bound from Python
NOT_BOUND_FROM_PYTHON = {
    "ntm_ipc_handle_bytes",   # the IPC handle size: xgmi.py passes a fixed 64-byte buffer
}

PROTOTYPE = re.compile(r"^NTM_API\s+(?P<ret>[\w\s]+?\**)\s*(?P<name>ntm_\w+)\((?P<args>[^()]*)\);", re.M)
SCALARS = {"int": "int", "unsigned": "uint", "unsigned int": "uint", "size_t": "size_t",
           "unsigned long long": "ulonglong", "float": "float", "double": "double"}
CTYPES = {ctypes.c_int: "int", ctypes.c_uint: "uint", ctypes.c_size_t: "size_t",
          ctypes.c_ulonglong: "ulonglong", ctypes.c_float: "float", ctypes.c_double: "double",
          ctypes.c_void_p: "pointer"}


# ctypes has ONE type for two C types of the same size and signedness: on LP64,
# c_size_t and c_ulonglong are the same object (c_ulong). Where that is so the two
# classes cannot be told apart from the Python side and count as one.
if ctypes.c_size_t is ctypes.c_ulonglong:
    SCALARS["size_t"] = "ulonglong"


def c_class(decl: str, is_return: bool = False) -> str:
    """The class of one C parameter or return type: a scalar's name, 'pointer', 'void' or 'char*'."""
    decl = decl.strip()
    if "*" in decl:
        base = decl[:decl.index("*")].replace("const", "").strip()
        return "char*" if is_return and base == "char" else "pointer"
    words = [w for w in decl.split() if w != "const"]
    if not is_return and len(words) > 1 and " ".join(words) not in SCALARS:
        words = words[:-1]                     # drop the parameter's name
    t = " ".join(words)
    return "void" if t == "void" else SCALARS[t]


def py_class(t, is_return: bool = False) -> str:
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "char*" if is_return else "pointer"
    if t in CTYPES:
        return CTYPES[t]
    assert issubclass(t, ctypes._Pointer), t   # a ctypes.POINTER(...)
    return "pointer"


def header_prototypes() -> dict:
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    protos = {}
    for m in PROTOTYPE.finditer(text):
        args = m.group("args").strip()
        argv = [] if args in ("", "void") else [c_class(a) for a in args.split(",")]
        assert m.group("name") not in protos, m.group("name")
        protos[m.group("name")] = (argv, c_class(m.group("ret"), is_return=True))
    # the parser saw every prototype line
    assert len(protos) == len(re.findall(r"^NTM_API\b", text, flags=re.M)) > 90
    return protos


def python_tables() -> dict:
    from nvidia_terraform_modules_amd.ops import _lib
    assert not set(_lib.SIGNATURES) & set(_lib.XGMI_SIGNATURES)
    return {**_lib.SIGNATURES, **_lib.XGMI_SIGNATURES}


def test_the_parser_reads_c():
    assert c_class("const void* const* in_ptrs") == "pointer" and c_class("unsigned* err") == "pointer"
    assert c_class("unsigned long long seed") == "ulonglong" and c_class("unsigned epoch") == "uint"
    assert c_class("size_t n") == CTYPES[ctypes.c_size_t] and c_class("double ratio") == "double"
    assert c_class("const char*", True) == "char*" and c_class("void", True) == "void"
    assert c_class("size_t", True) == CTYPES[ctypes.c_size_t] and c_class("char* json") == "pointer"
    p = header_prototypes()
    assert p["ntm_version"] == ([], "char*") and p["ntm_set_cus_override"] == (["int"], "void")
    assert p["ntm_fill_uniform_bf16"] == (["pointer", CTYPES[ctypes.c_size_t], "ulonglong", "float", "pointer"], "int")
    assert p["ntm_xgmi_signal_bytes"] == (["int"], CTYPES[ctypes.c_size_t])


def test_every_header_name_is_bound_or_listed():
    header, tables = set(header_prototypes()), set(python_tables())
    assert header - tables == NOT_BOUND_FROM_PYTHON
    assert not NOT_BOUND_FROM_PYTHON & tables


def test_every_python_name_is_in_the_header():
    assert set(python_tables()) - set(header_prototypes()) == set()


def test_common_names_agree_in_arity_and_class():
    header = header_prototypes()
    wrong = []
    for name, (argt, rest) in python_tables().items():
        want = header[name]
        got = ([py_class(t) for t in argt], py_class(rest, is_return=True))
        if got != want:
            wrong.append((name, got, want))
    assert not wrong, wrong


def test_the_header_covers_every_shipping_export_and_only_those():
    """Each NTM_API definition of the two shipping sources has a prototype (the compiler
    checks that they agree; this checks that none was left out, since a definition
    without a prototype still compiles) and the header declares nothing else."""
    defined = set()
    for f in ("ntm_validation.hip", "xgmi_allreduce.hip"):
        text = (SRC / f).read_text()
        assert '#include "ntm/abi.h"' in text and "#define NTM_API" not in text, f
        defined |= set(re.findall(r"^NTM_API\s+[\w\s]+?\**\s*(ntm_\w+)\(", text, flags=re.M))
    assert defined == set(header_prototypes())
    exp = (SRC / "ntm_experimental.hip").read_text()
    assert '#include "ntm/abi.h"' in exp and "#define NTM_API" not in exp


def test_the_job_binary_declares_nothing_by_hand():
    for f in sorted((SRC / "validate").iterdir()):
        if f.suffix in (".cpp", ".hpp", ".hip"):
            text = f.read_text()
            assert 'extern "C"' not in text and "kMaxRanks" not in text, f.name
            assert not re.search(r"^\s*(int|size_t|void)\s+ntm_\w+\(", text, flags=re.M), f.name
