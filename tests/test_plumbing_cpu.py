"""The plumbing every unit stands on, checked for all units at once (no GPU): the source manifest of fisher_rast._lib (what is
compiled, what the build id is taken over), the one compile recipe of __graft_entry__, and the prototype table against the headers."""
import ctypes
import inspect
import os
import re
import shutil

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc")


# ---- 1. the manifest ------------------------------------------------------------------------------------------------------------------

def _includes(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return [os.path.normpath(os.path.join(os.path.dirname(path), n)) for n in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, flags=re.M)]


def test_manifest_holds_every_unit_and_every_file_a_unit_includes():
    from fisher_rast import _lib
    on_disk = sorted(os.path.join(CSRC, n) for n in os.listdir(CSRC))
    assert _lib.UNITS == [f for f in on_disk if f.endswith(".hip")] and len(_lib.UNITS) >= 17
    assert [os.path.basename(h) for h in _lib.HEADERS] == ["fisher_rast.h", "fisher_occ.h"] and all(os.path.exists(h) for h in _lib.HEADERS)
    assert _lib.SOURCES == _lib.UNITS + [f for f in on_disk if f.endswith((".h", ".inc"))] + _lib.HEADERS
    assert len(set(_lib.SOURCES)) == len(_lib.SOURCES)
    assert os.path.join(CSRC, "fr_sortnet.h") in _lib.SOURCES          # once in neither list: an edit to the sort plan left the build id alone
    members, reached, todo = set(_lib.SOURCES), set(), list(_lib.UNITS)
    while todo:
        f = todo.pop()
        for inc in _includes(f):
            assert inc in members, f"{f} includes {inc}, which is not in _lib.SOURCES"
            if inc not in reached:
                reached.add(inc)
                todo.append(inc)
    assert os.path.join(CSRC, "fr_sortnet.h") in reached and set(_lib.HEADERS) <= reached          # ../../include/ is followed too


def test_build_id_changes_with_one_byte_of_any_member(tmp_path):
    from fisher_rast import _lib
    assert len({os.path.basename(f) for f in _lib.SOURCES}) == len(_lib.SOURCES)
    copies = [shutil.copy(f, tmp_path) for f in _lib.SOURCES]
    base = _lib.source_hash(copies)
    assert base == _lib.source_hash() and re.fullmatch(r"[0-9a-f]{16}", base)
    assert _lib.source_hash(copies + [str(tmp_path / "absent.h")]) is None
    for c in copies:
        data = open(c, "rb").read()
        open(c, "wb").write(data[:-1] + bytes([data[-1] ^ 1]))
        assert _lib.source_hash(copies) != base, os.path.basename(c)
        open(c, "wb").write(data)
    assert _lib.source_hash(copies) == base


# ---- 2. the compile recipe --------------------------------------------------------------------------------------------------------------

def test_build_compiles_exactly_the_units_with_the_one_set_of_flags():
    import __graft_entry__ as g
    from fisher_rast import _lib
    cmd = g.build_library("/nowhere/x.so", dry_run=True)
    assert not os.path.exists("/nowhere")
    assert [a for a in cmd if a.endswith((".hip", ".cpp", ".o"))] == _lib.UNITS
    assert cmd[1:1 + len(g.HIPCC_FLAGS)] == g.HIPCC_FLAGS and cmd[cmd.index("-o") + 1] == "/nowhere/x.so"
    assert f'-DFR_SRC_HASH="FRSRC:{_lib.source_hash()}"' in cmd
    variant = g.build_library("/nowhere/x.so", ["-DFR_AB"], dry_run=True)
    assert [a for a in variant if a not in cmd] == ["-DFR_AB"] and [a for a in variant if a != "-DFR_AB"] == cmd
    # build() goes through it and names no unit of its own
    src = inspect.getsource(g.build)
    assert "build_library(" in src and not re.search(r'"f\w+\.hip"', open(g.__file__).read())


def test_the_target_flag_is_written_in_one_file():
    """every tool that compiles the library or its kernels takes the flags from __graft_entry__.HIPCC_FLAGS: the target flag occurs in no
    other script (the build comments of the stand-alone microbenchmarks tools/*.hip are not scripts)"""
    found = []
    for d, dirs, files in os.walk(ROOT):
        dirs[:] = [x for x in dirs if not x.startswith((".", "_"))]
        for n in files:
            p = os.path.join(d, n)
            if n.endswith((".py", ".sh")) and not os.path.samefile(p, __file__) and "--offload-arch" in open(p, errors="replace").read():
                found.append(os.path.relpath(p, ROOT))
    assert found == ["__graft_entry__.py"]


# ---- 3. the prototype table -------------------------------------------------------------------------------------------------------------

C_KINDS = {"int": "i32", "int32_t": "i32", "int64_t": "i64", "uint32_t": "u32", "size_t": "size", "float": "f32", "double": "f64"}


def _c_kind(decl, named):
    """kind of one parameter declaration (or of a return type, named=False); a type outside the list is an error, never a pass"""
    if "*" in decl or "[" in decl or re.search(r"\bfr_stream_t\b", decl):
        return "pointer"
    words = [w for w in re.findall(r"\w+", decl) if w != "const"]
    if named and len(words) > 1:
        words = words[:-1]
    assert " ".join(words) in C_KINDS, f"no rule for the C type of {decl!r}"
    return C_KINDS[" ".join(words)]


def _ctypes_kind(t):
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "pointer"
    for kind, types in (("i32", (ctypes.c_int, ctypes.c_int32)), ("i64", (ctypes.c_int64,)), ("u32", (ctypes.c_uint32,)), ("size", (ctypes.c_size_t,)),
                        ("f32", (ctypes.c_float,)), ("f64", (ctypes.c_double,))):
        if any(t is x for x in types):
            return kind
    raise AssertionError(f"no rule for the ctypes type {t!r}")


def test_prototype_table_agrees_with_the_headers():
    from fisher_rast import _lib
    declared = sc.declared_exports(with_return=True)
    assert set(declared) == set(_lib.PROTOTYPES) and _lib.EXPORTS == tuple(_lib.PROTOTYPES) and len(_lib.EXPORTS) >= 96
    assert ctypes.sizeof(ctypes.c_int) == 4
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        ret, params = declared[name]
        assert ret in ("int", "int32_t", "size_t", "const char*"), (name, ret)
        assert _ctypes_kind(restype) == _c_kind(ret, named=False), (name, ret, restype)
        assert (restype is ctypes.c_char_p) == (ret == "const char*"), name
        params = [] if params.strip() in ("", "void") else params.split(",")
        assert len(argtypes or ()) == len(params), (name, len(argtypes or ()), len(params))
        for i, (a, p) in enumerate(zip(argtypes or (), params)):
            assert _ctypes_kind(a) == _c_kind(p, named=True), (name, i, p.strip(), a)


def test_the_kind_rules_refuse_what_they_do_not_know():
    import pytest
    for decl in ("fr_occ_cfg cfg", "long n", "unsigned n", "char c", "bool on"):
        with pytest.raises(AssertionError):
            _c_kind(decl, named=True)
    for t in (ctypes.c_int16, ctypes.c_uint8, ctypes.c_bool, None):
        with pytest.raises(AssertionError):
            _ctypes_kind(t)
    assert _c_kind("const float mean[3]", True) == _c_kind("fr_stream_t stream", True) == _c_kind("const fr_occ_cfg* cfg", True) == "pointer"
    assert _c_kind("int", True) == _c_kind("int32_t P", True) == "i32" and _c_kind("const char*", False) == "pointer"
