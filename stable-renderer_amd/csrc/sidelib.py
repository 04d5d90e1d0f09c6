"""Build the side libraries for gfx950 with hipcc: csrc/<name>/libsr_<name>.so, one translation unit each, linked in-tree next to
its source under a private name and renamed, carrying the hash of its sources (sr_<name>_source_hash).

Why they are libraries of their own: bench.py's recorded frame checksum and the recorded igemm traffic are stamped with the source
hash of libsr_hip.so (csrc/build.py).  Kept out of its source list, these leave that identity, and the records with it, alone.  For
the same reason this file loads csrc/build.py for hipcc() instead of touching it, and sr_side.h, not sr_common.h, is their prologue.

A new side library is one entry in LIBRARIES, one csrc/<name>/<name>.hip (which names itself with SR_SIDE / SR_SIDE_UC and gives
SR_<NAME>_SRC_HASH a default), one header sr_<name>.h and one binding module with a SYMBOLS table for _native.SideLibrary.  A public
library's ABI is described in INTEGRATION.md: its header lies under include/ and _lib_<name>.py binds it.  A private one has one
caller, this package: its header lies next to the source and _<name>.py binds it.  `shared` lists further headers under csrc/ that
the source includes; every file that reaches the compiler must be named here, or a stale library would pass for a current one.

    python stable-renderer_amd/csrc/sidelib.py [name ...] [--force]"""
import hashlib
import importlib.util
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]
SHARED = "sr_side.h"
CONV3 = ("conv3_pack.h",)         # the packed weight layout of the patch-stationary 3x3 convolutions
# name -> what cannot be derived from the name, in build order
LIBRARIES = {
    "tiled": dict(public=True), "resample": dict(public=True), "imgproc": dict(public=True),
    "ksteps": dict(public=False), "morph": dict(public=False), "esrgan": dict(public=False, shared=CONV3),
    "canny": dict(public=False), "taesd": dict(public=False, shared=CONV3), "compact": dict(public=False, shared=CONV3),
    "clip": dict(public=False), "t2i": dict(public=False), "inpaint": dict(public=False), "guidance": dict(public=False),
}


def names():
    return list(LIBRARIES)


def entry(name):
    """-> (directory, source, path of the header, hash macro); KeyError for an unknown name"""
    hdr = os.path.join(HERE, "..", "..", "include") if LIBRARIES[name]["public"] else os.path.join(HERE, name)
    return name, name + ".hip", os.path.join(hdr, "sr_%s.h" % name), "SR_%s_SRC_HASH" % name.upper()


def binding(name):
    """the module of the package that binds the library"""
    return ("_lib_" if LIBRARIES[name]["public"] else "_") + name


def sources(name):
    """every file of the repository the compiler reads for this library"""
    d, src, hdr, _ = entry(name)
    return [os.path.join(HERE, d, src), hdr, os.path.join(HERE, SHARED)] + [os.path.join(HERE, s) for s in LIBRARIES[name].get("shared", ())]


def lib_path(name):
    return os.path.join(HERE, entry(name)[0], "libsr_%s.so" % name)


def source_hash(name):
    """sha256 over sources(name) and the compile flags"""
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for fp in sources(name):
        h.update(os.path.basename(fp).encode())
        with open(fp, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:32]


def is_current(name):
    """the library in-tree carries the hash of these sources (looked up in the file's bytes: nothing stale is ever dlopen'ed)"""
    if not os.path.exists(lib_path(name)):
        return False
    with open(lib_path(name), "rb") as f:
        return source_hash(name).encode() in f.read()


def hipcc():
    spec = importlib.util.spec_from_file_location("sr_build", os.path.join(HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.hipcc()


def build(name, force=False):
    d, src, _, macro = entry(name)
    lib = lib_path(name)
    if force or not is_current(name):
        tmp = lib + ".tmp%d" % os.getpid()
        cmd = [hipcc()] + FLAGS + ['-D%s="%s"' % (macro, source_hash(name)), os.path.join(HERE, d, src), "-o", tmp]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        os.replace(tmp, lib)
    return lib


if __name__ == "__main__":
    for n in [a for a in sys.argv[1:] if a != "--force"] or names():
        print(build(n, force="--force" in sys.argv))
