"""Build libsr_imgproc.so (the image and mask filters: blur, sharpen, blend, composite, grow, feather, combine, include/sr_imgproc.h) for gfx950 with hipcc: one translation unit, linked in-tree next
to its source under a private name and renamed.  The image carries the hash of its sources (sr_imgproc_source_hash)."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libsr_imgproc.so")
SOURCE = "imgproc.hip"
HEADER = os.path.join("..", "..", "..", "include", "sr_imgproc.h")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def source_hash():
    h = hashlib.sha256()
    for f in (SOURCE, HEADER, os.path.basename(__file__)):
        h.update(f.encode())
        with open(os.path.join(HERE, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:32]


def is_current():
    """the library in-tree carries the hash of these sources (looked up in the file's bytes: nothing stale is ever dlopen'ed)"""
    if not os.path.exists(LIB):
        return False
    with open(LIB, "rb") as f:
        return source_hash().encode() in f.read()


def build(force=False):
    if force or not is_current():
        tmp = LIB + ".tmp%d" % os.getpid()
        cmd = [hipcc()] + FLAGS + [f'-DSR_IMGPROC_SRC_HASH="{source_hash()}"', os.path.join(HERE, SOURCE), "-o", tmp]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise RuntimeError("hipcc failed for %s:\n%s" % (SOURCE, r.stderr[-4000:]))
        os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
