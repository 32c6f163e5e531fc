"""The ctypes signature table of uninext_amd/_lib.py against the prototypes of every header under include/: names, argument
kinds (count and order) and return kinds.  ctypes checks none of this when the library is loaded -- a miscounted argument or
an `int` where the header says `size_t` is a corrupted call with raw device pointers -- so it is checked here (no GPU work)."""
import ctypes
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# prototypes per header in the tree when this test was written: a floor that keeps the parser from passing on nothing
PROTOTYPES_AT_LEAST = {"msda_hip.h": 24, "dynmask_hip.h": 8, "patch_embed_hip.h": 6, "linear_hip.h": 8, "layernorm_hip.h": 1,
                       "lsap_hip.h": 3, "matcher_cost_hip.h": 1, "ota_hip.h": 2, "biattn_hip.h": 3, "conv3x3_hip.h": 12}
C_KINDS = {"int": "int", "unsigned": "unsigned", "unsigned int": "unsigned", "size_t": "size_t", "long long": "long long",
           "float": "float", "double": "double"}
CTYPES_KINDS = {ctypes.c_int: "int", ctypes.c_uint: "unsigned", ctypes.c_size_t: "size_t", ctypes.c_longlong: "long long",
                ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_void_p: "pointer", ctypes.c_char_p: "pointer",
                None: "void"}
TYPE_WORDS = {"int", "unsigned", "long", "float", "double", "size_t", "void", "char", "short", "signed"}


def c_kind(decl, where, returns=False):
    """Kind of one C parameter (its name, if any, is dropped) or of a return type."""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if not returns and len(words) > 1 and words[-1] not in TYPE_WORDS:
        words.pop()
    ctype = " ".join(words)
    if returns and ctype == "void":
        return "void"
    assert ctype in C_KINDS, "%s: C type %r is not known to this test: add it to C_KINDS and to the table's aliases" % (where, ctype)
    return C_KINDS[ctype]


def ctypes_kind(t, where):
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return "pointer"
    assert t in CTYPES_KINDS, "%s: ctypes type %r is not known to this test" % (where, t)
    return CTYPES_KINDS[t]


def prototypes(path):
    """{name: (return kind, [argument kinds])} of every function declared in the header."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*?(?<!\\)$", " ", text, flags=re.M)                  # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    found = {}
    for statement in text.split(";"):
        statement = " ".join(statement.replace("}", " ").split())
        if "(" not in statement:
            assert not statement, "%s: not a prototype: %r" % (path, statement)
            continue
        m = re.fullmatch(r"([\w\s\*]+?)\s*\b(\w+)\s*\(([^()]*)\)", statement)
        assert m, "%s: cannot parse %r" % (path, statement)
        ret, name, args = m.groups()
        where = "%s: %s" % (os.path.basename(path), name)
        args = [] if args.strip() in ("", "void") else [c_kind(a, where) for a in args.split(",")]
        assert name not in found, where
        found[name] = (c_kind(ret, where, returns=True), args)
    return found


HEADERS = sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))


def test_parser_finds_todays_prototypes_in_all_ten_headers():
    got = {os.path.basename(h): len(prototypes(h)) for h in HEADERS}
    assert set(got) >= set(PROTOTYPES_AT_LEAST)
    for header, floor in PROTOTYPES_AT_LEAST.items():
        assert got[header] >= floor, (header, got[header])
    assert sum(got.values()) >= 68


def test_every_header_has_a_group_and_every_group_a_header():
    from uninext_amd import _lib
    assert set(_lib._SIGNATURES) == {os.path.basename(h) for h in HEADERS}
    names = [n for group in _lib._SIGNATURES.values() for n in group]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("header", [os.path.basename(h) for h in HEADERS])
def test_table_rows_equal_the_header(header):
    from uninext_amd import _lib
    declared = prototypes(os.path.join(ROOT, "include", header))
    group = _lib._SIGNATURES[header]
    assert set(declared) == set(group)
    for name, (restype, argtypes) in group.items():
        where = "%s: %s" % (header, name)
        row = (ctypes_kind(restype, where), [ctypes_kind(t, where) for t in argtypes])
        assert row == declared[name], "%s: table %s, header %s" % (where, row, declared[name])


def test_groups_are_the_export_tuples():
    from uninext_amd import _lib
    tuples = {"msda_hip.h": _lib.EXPORTS, "dynmask_hip.h": _lib.DYNMASK_EXPORTS, "patch_embed_hip.h": _lib.PATCH_EMBED_EXPORTS,
              "linear_hip.h": _lib.LINEAR_EXPORTS, "layernorm_hip.h": _lib.LAYERNORM_EXPORTS, "lsap_hip.h": _lib.LSAP_EXPORTS,
              "matcher_cost_hip.h": _lib.MATCHER_COST_EXPORTS, "ota_hip.h": _lib.OTA_EXPORTS, "biattn_hip.h": _lib.BIATTN_EXPORTS,
              "conv3x3_hip.h": _lib.CONV3X3_EXPORTS}
    assert set(tuples) == set(_lib._SIGNATURES)
    for header, exports in tuples.items():
        assert sorted(exports) == sorted(_lib._SIGNATURES[header]) and len(exports) == len(set(exports))


def test_loaded_library_carries_every_row():
    from uninext_amd import _lib
    lib = _lib.load()
    for header, group in _lib._SIGNATURES.items():
        for name, (restype, argtypes) in group.items():
            fn = getattr(lib, name)
            assert fn.argtypes is not None, name                     # a function load() skipped has none
            assert list(fn.argtypes) == list(argtypes) and fn.restype is restype, name
