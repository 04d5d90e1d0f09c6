"""The shared loader (_native.py) on the side libraries of csrc/sidelib.py: what tests/test_host_logic.py checks for libsr_hip.so
(a stale or missing library is refused, never loaded, and nothing stands in for it) holds for each of them, and the registry, the
binding modules and the headers name the same libraries.  No GPU; nothing is built or dlopen'ed."""
import importlib
import os

import pytest

from stable_renderer_amd import _native
from stable_renderer_amd._lib import SrHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = ("tiled", "resample", "imgproc")


def _side(monkeypatch, name):
    """the module's SideLibrary, unloaded, in a process that may neither build nor dlopen"""
    side = importlib.import_module("stable_renderer_amd._lib_" + name)._side

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


def test_registry_modules_and_headers_name_the_same_libraries():
    sidelib = _native.sidelib()
    assert tuple(sidelib.REGISTRY) == SIDE
    headers = sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "sr_hip.h")
    assert headers == sorted(f"sr_{n}.h" for n in SIDE)
    pkg = os.path.dirname(_native.__file__)
    assert sorted(f for f in os.listdir(pkg) if f.startswith("_lib_")) == sorted(f"_lib_{n}.py" for n in SIDE)
    for name, (d, src, hdr, macro) in sidelib.REGISTRY.items():
        mod = importlib.import_module("stable_renderer_amd._lib_" + name)
        assert hdr == f"sr_{name}.h" and macro == f"SR_{name.upper()}_SRC_HASH"
        assert os.path.exists(os.path.join(_native.CSRC, d, src))
        assert mod._side.name == name and mod.LIB_PATH == sidelib.lib_path(name) == os.path.join(_native.CSRC, d, f"libsr_{name}.so")
        assert {f"sr_{name}_last_error", f"sr_{name}_source_hash"} <= set(mod.SYMBOLS)
        with open(os.path.join(_native.CSRC, d, src)) as f:
            text = f.read()
        assert f"#define SR_SIDE {name}\n" in text and f"#define SR_SIDE_UC {name.upper()}\n" in text and f'"../../../include/{hdr}"' in text
