"""Build the side libraries for gfx950 with hipcc: libsr_tiled.so (the tiled VAE), libsr_resample.so (common_upscale) and
libsr_imgproc.so (the image and mask filters).  Each is one translation unit, linked in-tree next to its source under a private
name and renamed, and carries the hash of its sources (sr_<name>_source_hash).

Why they are libraries of their own: bench.py's recorded frame checksum and the recorded igemm traffic are stamped with the source
hash of libsr_hip.so (csrc/build.py).  These are bandwidth-bound helpers around its launch plans; kept out of its source list,
they leave that identity, and the records with it, alone.  For the same reason this file loads csrc/build.py for hipcc() instead
of touching it, and sr_side.h, not sr_common.h, is their shared prologue.

A new side library is one entry here, one .hip, one header under include/ and one SYMBOLS table bound by _native.SideLibrary.

PRIVATE holds the side libraries whose ABI only this package calls (no call site in the reference, nothing for INTEGRATION.md to
describe): their header lies next to the source, not under include/, and their binding module is not named _lib_*.py.  They are
built, hashed and loaded by the same rules; every function here resolves a name in either table.

PRIVATE_NODES is a third table of the same form as PRIVATE, for the private libraries behind graph nodes (libsr_morph.so: Morphology
and Porter-Duff compositing).  It exists because the contents of the two older tables are pinned by tests; names() lists all three.

PRIVATE_MODELS is a fourth table of the same form, for the private libraries that run a whole model (libsr_esrgan.so: the upscale
models).  names() and the three older tables are pinned by tests, so all_names() = names() + this table.

PRIVATE_EXTRA is the fifth table of the same form and the open-ended one: all_names() and the four older tables are pinned by tests,
so every later private library joins this table (libsr_canny.so is the first, libsr_taesd.so, the TAESD tiny autoencoder, the
second, libsr_compact.so, the Real-ESRGAN compact upscale models, the third, libsr_clip.so, the CLIP text encoder, the fourth, libsr_t2i.so, the
T2I-Adapter control network, the fifth, libsr_inpaint.so, masked (inpaint) sampling, the sixth,
libsr_guidance.so, model sampling and guidance, the seventh), and no test pins its length or its full content.
every_name() = all_names() + this table is what builds everything.

    python stable-renderer_amd/csrc/sidelib.py [name ...] [--force]"""
import hashlib
import importlib.util
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]
SHARED = "sr_side.h"
# name -> (directory, source, public header under include/, hash macro)
REGISTRY = {
    "tiled": ("tiled", "tiled.hip", "sr_tiled.h", "SR_TILED_SRC_HASH"),
    "resample": ("resample", "resample.hip", "sr_resample.h", "SR_RESAMPLE_SRC_HASH"),
    "imgproc": ("imgproc", "imgproc.hip", "sr_imgproc.h", "SR_IMGPROC_SRC_HASH"),
}
# name -> (directory, source, private header next to the source, hash macro)
PRIVATE = {
    "ksteps": ("ksteps", "ksteps.hip", "sr_ksteps.h", "SR_KSTEPS_SRC_HASH"),
}
# name -> (directory, source, private header next to the source, hash macro)
PRIVATE_NODES = {
    "morph": ("morph", "morph.hip", "sr_morph.h", "SR_MORPH_SRC_HASH"),
}
# name -> (directory, source, private header next to the source, hash macro)
PRIVATE_MODELS = {
    "esrgan": ("esrgan", "esrgan.hip", "sr_esrgan.h", "SR_ESRGAN_SRC_HASH"),
}
# name -> (directory, source, private header next to the source, hash macro); later private libraries join this table
PRIVATE_EXTRA = {
    "canny": ("canny", "canny.hip", "sr_canny.h", "SR_CANNY_SRC_HASH"),
    "taesd": ("taesd", "taesd.hip", "sr_taesd.h", "SR_TAESD_SRC_HASH"),
    "compact": ("compact", "compact.hip", "sr_compact.h", "SR_COMPACT_SRC_HASH"),
    "clip": ("clip", "clip.hip", "sr_clip.h", "SR_CLIP_SRC_HASH"),
    "t2i": ("t2i", "t2i.hip", "sr_t2i.h", "SR_T2I_SRC_HASH"),
    "inpaint": ("inpaint", "inpaint.hip", "sr_inpaint.h", "SR_INPAINT_SRC_HASH"),
    "guidance": ("guidance", "guidance.hip", "sr_guidance.h", "SR_GUIDANCE_SRC_HASH"),
}


def names():
    """every side library: the three tables' names, in order"""
    return list(REGISTRY) + list(PRIVATE) + list(PRIVATE_NODES)


def all_names():
    """names() and the model libraries of PRIVATE_MODELS"""
    return names() + list(PRIVATE_MODELS)


def every_name():
    """all_names() and the libraries of PRIVATE_EXTRA: everything sidelib builds"""
    return all_names() + list(PRIVATE_EXTRA)


def entry(name):
    """-> (directory, source, path of the header, hash macro) of a public or a private side library"""
    if name in REGISTRY:
        d, src, hdr, macro = REGISTRY[name]
        return d, src, os.path.join(HERE, "..", "..", "include", hdr), macro
    for table in (PRIVATE, PRIVATE_NODES, PRIVATE_MODELS, PRIVATE_EXTRA):
        if name in table:
            d, src, hdr, macro = table[name]
            break
    else:
        raise KeyError(name)
    return d, src, os.path.join(HERE, d, hdr), macro


def lib_path(name):
    return os.path.join(HERE, entry(name)[0], "libsr_%s.so" % name)


def source_hash(name):
    """sha256 over the source, its header (wherever it lies), the shared prologue and this file (the flags live here)"""
    d, src, hdr, _ = entry(name)
    h = hashlib.sha256()
    for fp in (os.path.join(HERE, d, src), hdr, os.path.join(HERE, SHARED), os.path.abspath(__file__)):
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
    for n in [a for a in sys.argv[1:] if a != "--force"] or every_name():
        print(build(n, force="--force" in sys.argv))
