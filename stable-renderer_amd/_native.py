"""The one loader of the native libraries: libsr_hip.so (csrc/build.py, bound by _lib.py) and the side libraries of
csrc/sidelib.py (each bound by the module sidelib.binding(name) names).  A library must have been built from the sources lying
next to it: a missing or stale one is rebuilt when hipcc is there and refused otherwise -- it is never loaded silently (a stale .so
was tested once: commit e818dd3), and there is no CPU fallback."""
import ctypes as C
import functools
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
_NO_FALLBACK = "there is no CPU fallback for the product path"


class SrHipError(RuntimeError):
    pass


def load_module(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bind(L, symbols):
    for name, (res, args) in symbols.items():
        fn = getattr(L, name)          # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    return L


def load(path, symbols, bm, hash_symbol, rebuild):
    """dlopen `path` and bind `symbols`.  bm is the library's build recipe: source_hash() of the sources lying in-tree,
    built_hash() of the library lying in-tree (None if unknown) and build(); `rebuild` is the command a person would run."""
    so = os.path.basename(path)
    want = bm.source_hash()
    # Fast path without writing anything (a read-only install, or a current library shipped without what git ignores under
    # csrc/_obj): the library in-tree already carries the hash of these sources.
    # (found by looking for the hash string in the file's bytes: dlopen'ing a stale image would pin it in this process)
    L = None
    if os.path.exists(path) and bm.built_hash() in (None, want):
        try:
            with open(path, "rb") as f:
                current = want.encode() in f.read()
            if current:
                L = bind(C.CDLL(path), symbols)
        except (OSError, AttributeError):
            L = None
    if L is None:
        # One builder at a time (ranks of bench --gpus N, spawned test workers and parallel pytest all land here with the same
        # stale hash): the lock covers the hash check, the compile and the rename of the linked file.
        import fcntl
        try:
            os.makedirs(os.path.join(CSRC, "_obj"), exist_ok=True)
            lock = open(os.path.join(CSRC, "_obj", ".build.lock"), "w")
        except OSError as e:
            raise SrHipError(f"{so} is stale or missing (sources are {want}) and {CSRC} is not writable for a rebuild: {e}; "
                             f"{_NO_FALLBACK}") from e
        with lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                have = bm.built_hash()
                if have != want:
                    stale = f"{so} is stale or missing (built from {have}, sources are {want})"
                    if os.environ.get("SR_NO_REBUILD") == "1":
                        raise SrHipError(f"{stale} and SR_NO_REBUILD=1; {_NO_FALLBACK}")
                    try:
                        bm.build()
                    except Exception as e:         # no hipcc, compile error
                        raise SrHipError(f"{stale} and the rebuild failed: {e}\nrun `{rebuild}`; {_NO_FALLBACK}") from e
                if not os.path.exists(path):
                    raise SrHipError(f"{path} not built; {_NO_FALLBACK}")
                L = bind(C.CDLL(path), symbols)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    have = getattr(L, hash_symbol)().decode()
    if have != want:
        raise SrHipError(f"{so} (built from {have}) does not match its sources ({want}): remove it and {os.path.join(CSRC, '_obj')}, "
                         f"then run `{rebuild}`")
    return L


def fail(rc, so, text):
    raise SrHipError("%s: %s (code %d)" % (so, text.decode(errors="replace"), rc))


@functools.lru_cache(maxsize=None)
def sidelib():
    return load_module("sr_sidelib", os.path.join(CSRC, "sidelib.py"))


class SideLibrary:
    """lib() / check() / path of one entry of csrc/sidelib.py's registry; it is its own build recipe for load()"""

    def __init__(self, name, symbols):
        self.name, self.symbols, self.path, self._lib = name, symbols, sidelib().lib_path(name), None

    def source_hash(self):
        return sidelib().source_hash(self.name)

    def built_hash(self):
        return sidelib().source_hash(self.name) if sidelib().is_current(self.name) else None

    def build(self):
        return sidelib().build(self.name)

    def lib(self):
        if self._lib is None:
            self._lib = load(self.path, self.symbols, self, f"sr_{self.name}_source_hash",
                             f"python stable-renderer_amd/csrc/sidelib.py {self.name}")
        return self._lib

    def check(self, rc):
        if rc != 0:
            fail(rc, "libsr_" + self.name, getattr(self.lib(), f"sr_{self.name}_last_error")())
