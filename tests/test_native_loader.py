"""The shared loader (_native.py) on the side libraries of csrc/sidelib.py: what tests/test_host_logic.py checks for libsr_hip.so
(a stale or missing library is refused, never loaded, and nothing stands in for it) holds for each of them; the table, the binding
modules, the headers and the sources name the same libraries; the source hash covers everything that reaches the compiler.  This is
the one place that pins the list of libraries.  No GPU; nothing is built or dlopen'ed."""
import importlib
import os
import re

import pytest

from stable_renderer_amd import _native
from stable_renderer_amd._lib import SrHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
entry_points = _native.load_module("sr_entry_points", os.path.join(ROOT, "__graft_entry__.py"))
PUBLIC = ("tiled", "resample", "imgproc")
SIDE = PUBLIC + ("ksteps", "morph", "esrgan", "canny", "taesd", "compact", "clip", "t2i", "inpaint", "guidance")
CONV3_PACK = ("esrgan", "taesd", "compact")      # the libraries whose hash csrc/conv3_pack.h enters, and no other's
sidelib = _native.sidelib()


def _binding(name):
    return importlib.import_module("stable_renderer_amd." + sidelib.binding(name))


def _side(monkeypatch, name):
    """the module's SideLibrary, unloaded, in a process that may neither build nor dlopen"""
    side = _binding(name)._side

    def never(*a, **k):
        raise AssertionError("the loader must refuse before it builds or loads anything")
    monkeypatch.setattr(side, "_lib", None)
    monkeypatch.setattr(side, "build", never)
    monkeypatch.setattr(_native.C, "CDLL", never)
    monkeypatch.setenv("SR_NO_REBUILD", "1")
    return side


@pytest.mark.parametrize("name", SIDE)
def test_stale_side_library_is_refused(monkeypatch, name):
    side = _side(monkeypatch, name)
    real = side.source_hash()
    monkeypatch.setattr(side, "source_hash", lambda: "deadbeef" + real[8:])
    with pytest.raises(SrHipError, match="stale or missing") as e:
        side.lib()
    assert f"libsr_{name}.so" in str(e.value) and "deadbeef" + real[8:] in str(e.value) and "no CPU fallback" in str(e.value)


@pytest.mark.parametrize("name", SIDE)
def test_no_cpu_fallback_without_side_library(monkeypatch, name):
    side = _side(monkeypatch, name)
    monkeypatch.setattr(side, "path", f"/nonexistent/libsr_{name}.so")
    with pytest.raises(SrHipError, match="no CPU fallback"):
        side.lib()


def test_the_table_is_the_thirteen_libraries_in_order():
    assert sidelib.names() == list(SIDE) == list(sidelib.LIBRARIES)
    assert tuple(n for n in sidelib.names() if sidelib.LIBRARIES[n]["public"]) == PUBLIC == SIDE[:3]
    assert sorted(os.listdir(os.path.join(ROOT, "include"))) == sorted(["sr_hip.h"] + [f"sr_{n}.h" for n in PUBLIC])
    pkg = os.path.dirname(_native.__file__)
    assert sorted(f for f in os.listdir(pkg) if f.startswith("_lib_")) == sorted(f"_lib_{n}.py" for n in PUBLIC)
    hashes = [sidelib.source_hash(n) for n in SIDE]
    assert all(re.fullmatch(r"[0-9a-f]{32}", h) for h in hashes) and len(set(hashes)) == len(hashes)
    with pytest.raises(KeyError):
        sidelib.entry("no_such_library")


@pytest.mark.parametrize("name", SIDE)
def test_table_module_header_and_source_name_the_same_library(name):
    public = name in PUBLIC
    d, src, hdr, macro = sidelib.entry(name)
    assert (d, src, os.path.basename(hdr), macro) == (name, f"{name}.hip", f"sr_{name}.h", f"SR_{name.upper()}_SRC_HASH")
    assert os.path.exists(os.path.join(_native.CSRC, d, src)) and os.path.exists(hdr)
    assert os.path.samefile(os.path.dirname(hdr), os.path.join(ROOT, "include") if public else os.path.join(_native.CSRC, name))
    assert sidelib.binding(name) == ("_lib_" if public else "_") + name
    assert public or not os.path.exists(os.path.join(os.path.dirname(_native.__file__), f"_lib_{name}.py"))
    mod = _binding(name)
    assert mod._side.name == name and mod.LIB_PATH == sidelib.lib_path(name) == os.path.join(_native.CSRC, name, f"libsr_{name}.so")
    assert {f"sr_{name}_last_error", f"sr_{name}_source_hash"} <= set(mod.SYMBOLS)
    with open(os.path.join(_native.CSRC, d, src)) as f:
        text = f.read()
    assert f"#define SR_SIDE {name}\n" in text and f"#define SR_SIDE_UC {name.upper()}\n" in text and '"../sr_side.h"' in text
    assert ('"../../../include/' if public else '"') + f'sr_{name}.h"' in text


def _included(path, seen):
    """every file of the repository that `path` pulls in with a quoted #include, transitively"""
    with open(path) as f:
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
            fp = os.path.realpath(os.path.join(os.path.dirname(path), inc))
            if os.path.exists(fp) and fp not in seen:
                seen.add(fp)
                _included(fp, seen)
    return seen


@pytest.mark.parametrize("name", SIDE)
def test_source_hash_reads_every_file_the_source_includes(monkeypatch, name):
    d, src, _, _ = sidelib.entry(name)
    src = os.path.realpath(os.path.join(_native.CSRC, d, src))
    read, real_open = set(), open

    def spy(path, *a, **k):
        read.add(os.path.realpath(path))
        return real_open(path, *a, **k)
    monkeypatch.setattr(sidelib, "open", spy, raising=False)
    sidelib.source_hash(name)
    monkeypatch.undo()
    assert _included(src, {src}) <= read
    shared = {os.path.realpath(os.path.join(_native.CSRC, "conv3_pack.h"))} if name in CONV3_PACK else set()
    assert {f for f in read if os.path.basename(f) == "conv3_pack.h"} == shared
    assert os.path.realpath(sidelib.__file__) not in read          # entering a library leaves the others current


def test_flags_enter_every_hash(monkeypatch):
    before = {n: sidelib.source_hash(n) for n in SIDE}
    monkeypatch.setattr(sidelib, "FLAGS", sidelib.FLAGS + ["-DANOTHER"])
    after = {n: sidelib.source_hash(n) for n in SIDE}
    assert all(before[n] != after[n] for n in SIDE)


def test_entry_build_goes_through_names(monkeypatch):
    """__graft_entry__.build() builds and binds every library of names(): a new entry of the table is built with the rest"""
    from stable_renderer_amd import _lib
    built, bound = [], []

    class Stub:
        def lib(self):
            pass

    def import_module(mod):
        bound.append(mod)
        return Stub()
    monkeypatch.setattr(sidelib, "build", lambda name, force=False: built.append(name) or __file__)
    monkeypatch.setattr(_lib, "_build_module", lambda: type("B", (), {"build": staticmethod(lambda verbose=False: __file__)}))
    monkeypatch.setattr(_lib, "lib", lambda: None)
    monkeypatch.setattr(entry_points.importlib, "import_module", import_module)
    monkeypatch.setattr(entry_points.subprocess, "run", lambda *a, **k: None)
    entry_points.build()
    assert built == list(SIDE) and bound == ["stable_renderer_amd." + sidelib.binding(n) for n in SIDE]
