"""Operator-level C ABI (include/sr_hip.h: sr_model_load / sr_unet_forward / sr_vae_decode): a UNet and a VAE decoder lowered and
tuned by the Python host are exported as model bundles (bundle.py) and then run by a CHILD PROCESS THAT IMPORTS NEITHER torch NOR
this package -- ctypes on libsr_hip.so and numpy only, the stand-in for a C++ / Go / Rust host -- which must reproduce the Python
path's outputs bit for bit (same kernels, same pinned tiles; UNetModel.forward openaimodel.py:841-946, VAE.decode sd.py:329-346)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

CHILD = r'''
import ctypes as C, sys, numpy as np
assert "torch" not in sys.modules
lib = C.CDLL(sys.argv[1])
vp = C.c_void_p
lib.sr_last_error.restype = C.c_char_p
lib.sr_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
lib.sr_unet_forward.argtypes = [vp, vp, vp, vp, vp, vp]
lib.sr_vae_decode.argtypes = [vp, vp, vp, vp]
lib.sr_model_write.argtypes = [vp, C.c_char_p, vp, vp]
lib.sr_model_io.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int64)]
lib.sr_model_free.argtypes = [vp]
def ck(rc):
    assert rc == 0, lib.sr_last_error().decode()
d = np.load(sys.argv[2])
m = vp()
ck(lib.sr_model_load(sys.argv[3].encode(), C.byref(m)))
x, t, ctx = np.ascontiguousarray(d["x"]), np.ascontiguousarray(d["t"]), np.ascontiguousarray(d["ctx"])
out = np.empty_like(x)
nb = C.c_int64()
ck(lib.sr_model_io(m, b"ctx", None, C.byref(nb)))
assert nb.value == ctx.nbytes, (nb.value, ctx.nbytes)
if "inject" in d.files:
    inj = np.ascontiguousarray(d["inject"].astype(np.int32))
    ck(lib.sr_model_write(m, b"inject", inj.ctypes.data_as(vp), None))
ck(lib.sr_unet_forward(m, x.ctypes.data_as(vp), t.ctypes.data_as(vp), ctx.ctypes.data_as(vp), out.ctypes.data_as(vp), None))
ck(lib.sr_device_sync())
out2 = np.empty_like(x)                      # second evaluation, same prompt: ctx = NULL keeps the projected K / V
ck(lib.sr_unet_forward(m, x.ctypes.data_as(vp), t.ctypes.data_as(vp), None, out2.ctypes.data_as(vp), None))
ck(lib.sr_device_sync())
ck(lib.sr_model_free(m))
v = vp()
ck(lib.sr_model_load(sys.argv[4].encode(), C.byref(v)))
z = np.ascontiguousarray(d["z"])
img = np.empty(tuple(d["img_shape"]), np.float32)
ck(lib.sr_vae_decode(v, z.ctypes.data_as(vp), img.ctypes.data_as(vp), None))
ck(lib.sr_device_sync())
ck(lib.sr_model_free(v))
bad = vp()
assert lib.sr_model_load(b"/nonexistent.srm", C.byref(bad)) != 0 and b"cannot open" in lib.sr_last_error()
np.savez(sys.argv[5], out=out, out2=out2, img=img)
'''


def _sd(name, seed):
    from stable_renderer_amd import synth
    with open(os.path.join(GOLD, name)) as f:
        k = json.load(f)
    return synth.synth_state_dict([(n, tuple(s)) for n, s in k["names_shapes"]], seed=seed, norm_names=k["norm_names"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_unet_and_vae_bundles_run_from_a_process_without_torch(tmp_path, dtype):
    from stable_renderer_amd import _lib, bundle
    from stable_renderer_amd.unet import SD15_CFG, UNet
    from stable_renderer_amd.vae import VAEDecoder
    cfg = dict(SD15_CFG, model_channels=64, context_dim=64)
    net = UNet(_sd("unet_tiny_keys.json", 1), cfg, dtype=dtype)
    g = torch.Generator().manual_seed(5)
    B, h, w = 4, 16, 16
    x, t, ctx = torch.randn(B, 4, h, w, generator=g), torch.tensor([981.0] * B), torch.randn(B, 77, 64, generator=g)
    p = net.build(B, h, w, inject_idx=[2], n_ctx=77)
    p["x"].copy_(x)
    p["t"].copy_(t)
    p["ctx"].copy_(ctx.to(dtype))
    p["prologue"].run()
    p["step"].run()
    torch.cuda.synchronize()
    ref = p["out"].cpu().numpy().copy()
    info = bundle.export_unet(str(tmp_path / "unet.srm"), net, p)
    assert info["saved"] > 100                                 # the packed weights travelled
    dec = VAEDecoder(_sd("vae_dec_keys.json", 2), dtype=dtype)
    z = torch.randn(2, 4, 8, 8, generator=g)
    vp_ = dec.build(2, 8, 8)
    vp_["z"].copy_(z)
    vp_["plan"].run()
    torch.cuda.synchronize()
    ref_img = vp_["img"].cpu().numpy().copy()
    bundle.export_vae(str(tmp_path / "vae.srm"), dec, vp_)
    np.savez(tmp_path / "in.npz", x=x.numpy(), t=t.numpy(), ctx=ctx.to(dtype).numpy(), inject=np.array([2]), z=z.numpy(),
             img_shape=np.array(ref_img.shape))
    child = tmp_path / "child.py"
    child.write_text(CHILD)
    env = dict(os.environ, PYTHONPATH="")
    r = subprocess.run([sys.executable, str(child), _lib.LIB_PATH, str(tmp_path / "in.npz"), str(tmp_path / "unet.srm"),
                        str(tmp_path / "vae.srm"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    o = np.load(tmp_path / "out.npz")
    assert np.array_equal(o["out"], ref) and np.array_equal(o["out2"], ref)     # same kernels, same tiles: bit for bit
    assert np.array_equal(o["img"], ref_img)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.1


# ------------------------------------------------------------------------------------------------------------------------------------
# The loader against everything else a bundle can be: other topologies, dtypes and shapes; hostile files; the run-time error paths;
# streams and lifetimes.  Every bundle exported here is first judged by the host-only reader (csrc/bundle_file.h through
# tests/native/bundle_check_main.cpp, plain build), which must accept what bundle.export_bundle writes and report, for every
# relocation, the extent tests/bundle_ref.py computes on its own.  NO TEST RUNS A MUTATED BUNDLE: a hostile file is only ever loaded.
import ctypes as C
import struct

import bundle_ref as R

CHILD2 = r'''
import ctypes as C, json, sys, numpy as np
assert "torch" not in sys.modules
lib = C.CDLL(sys.argv[1])
spec = json.load(open(sys.argv[2]))
vp = C.c_void_p
lib.sr_last_error.restype = C.c_char_p
lib.sr_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
lib.sr_unet_forward.argtypes = [vp, vp, vp, vp, vp, vp]
lib.sr_vae_decode.argtypes = [vp, vp, vp, vp]
lib.sr_model_write.argtypes = [vp, C.c_char_p, vp, vp]
lib.sr_model_io.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.POINTER(C.c_int64)]
lib.sr_model_free.argtypes = [vp]
def ck(rc):
    assert rc == 0, lib.sr_last_error().decode()
d = np.load(spec["npz"])
m = vp()
ck(lib.sr_model_load(spec["model"].encode(), C.byref(m)))
for name, want in spec["io"].items():
    nb, ptr = C.c_int64(), vp()
    ck(lib.sr_model_io(m, name.encode(), C.byref(ptr), C.byref(nb)))
    assert nb.value == want and ptr.value, (name, nb.value, want)
res = {}
if spec["kind"] == "unet":
    x, t, ctx = (np.ascontiguousarray(d[k]) for k in ("x", "t", "ctx"))
    for extra in ("y", "inject"):
        if extra in d.files:
            a = np.ascontiguousarray(d[extra])
            ck(lib.sr_model_write(m, extra.encode(), a.ctypes.data_as(vp), None))
    out, out2 = np.empty_like(x), np.empty_like(x)
    ck(lib.sr_unet_forward(m, x.ctypes.data_as(vp), t.ctypes.data_as(vp), ctx.ctypes.data_as(vp), out.ctypes.data_as(vp), None))
    ck(lib.sr_device_sync())
    ck(lib.sr_unet_forward(m, x.ctypes.data_as(vp), t.ctypes.data_as(vp), None, out2.ctypes.data_as(vp), None))
    ck(lib.sr_device_sync())
    res = dict(out=out, out2=out2)
else:
    z = np.ascontiguousarray(d["z"])
    img = np.empty(tuple(d["img_shape"]), np.float32)
    ck(lib.sr_vae_decode(m, z.ctypes.data_as(vp), img.ctypes.data_as(vp), None))
    ck(lib.sr_device_sync())
    res = dict(out=img, out2=img)
ck(lib.sr_model_free(m))
np.savez(spec["out"], **res)
'''

_CASES = {
    # name: (kind, config, dtype, B, h, w, inject)
    "sd15_f16_inject": ("unet", "sd15", torch.float16, 4, 16, 16, [2]),
    "sd15_f32_plain": ("unet", "sd15", torch.float32, 2, 16, 16, None),
    "sd15_f16_odd": ("unet", "sd15", torch.float16, 2, 10, 12, None),
    "sd15_f32_odd_inject": ("unet", "sd15", torch.float32, 3, 10, 12, [0]),
    "sdxl_f16_inject": ("unet", "sdxl", torch.float16, 3, 16, 16, [1]),
    "sdxl_f32_plain": ("unet", "sdxl", torch.float32, 2, 16, 16, None),
    "vae_f16_8x8": ("vae", None, torch.float16, 2, 8, 8, None),
    "vae_f16_13x2": ("vae", None, torch.float16, 2, 13, 2, None),       # 26 keys: the mid attention pads them (test_gpu_vae_tiled.py)
    "vae_f32_13x2": ("vae", None, torch.float32, 2, 13, 2, None),
}
_BUILT = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("bundles")


@pytest.fixture(scope="module")
def driver(workdir):
    return R.build_driver(workdir, sanitize=False)             # plain: sanitizer runs do not belong where a GPU is


def _case(name, workdir):
    """export the bundle of a case once: -> dict(path, npz, ref, io = {window: bytes}, inputs)"""
    if name in _BUILT:
        return _BUILT[name]
    from stable_renderer_amd import bundle
    kind, cfgname, dtype, B, h, w, inject = _CASES[name]
    g = torch.Generator().manual_seed(sum(name.encode()))
    path, npz = str(workdir / (name + ".srm")), str(workdir / (name + ".npz"))
    if kind == "unet":
        from stable_renderer_amd.unet import SD15_CFG, UNet
        if cfgname == "sd15":
            cfg, keys, seed = dict(SD15_CFG, model_channels=64, context_dim=64), "unet_tiny_keys.json", 1
        else:
            from test_gpu_models import SDXL_TINY
            cfg, keys, seed = SDXL_TINY, "unet_sdxl_tiny_keys.json", 4
        net = UNet(_sd(keys, seed), cfg, dtype=dtype)
        x, t = torch.randn(B, 4, h, w, generator=g), torch.tensor([981.0, 500.0, 37.0, 1.0][:B])
        ctx = torch.randn(B, 77, cfg["context_dim"], generator=g).to(dtype)
        p = net.build(B, h, w, inject_idx=inject, n_ctx=77)
        p["x"].copy_(x)
        p["t"].copy_(t)
        p["ctx"].copy_(ctx)
        arrays = dict(x=x.numpy(), t=t.numpy(), ctx=ctx.numpy())
        if p.get("y") is not None:                              # SDXL family: the vector conditioning, padded to the K-step
            y = torch.zeros(p["y"].shape, dtype=dtype)
            y[:, :cfg["adm_in_channels"]] = torch.randn(B, cfg["adm_in_channels"], generator=g).to(dtype)
            p["y"].copy_(y)
            arrays["y"] = y.numpy()
        if inject is not None:
            arrays["inject"] = np.array(inject, np.int32)
        p["prologue"].run()
        p["step"].run()
        torch.cuda.synchronize()
        ref = p["out"].cpu().numpy().copy()
        if p.get("y") is not None:
            p["y"].zero_()                                      # the file must not carry it: the host writes it (sr_model_write)
        bundle.export_unet(path, net, p)
        io = {k: p[k].numel() * p[k].element_size() for k in ("x", "t", "ctx", "out", "y", "inject", "inject_err") if p.get(k) is not None}
        keep = (net, p)
    else:
        from stable_renderer_amd.vae import VAEDecoder
        dec = VAEDecoder(_sd("vae_dec_keys.json", 2), dtype=dtype)
        z = torch.randn(B, 4, h, w, generator=g)
        p = dec.build(B, h, w)
        p["z"].copy_(z)
        p["plan"].run()
        torch.cuda.synchronize()
        ref = p["img"].cpu().numpy().copy()
        bundle.export_vae(path, dec, p)
        arrays = dict(z=z.numpy(), img_shape=np.array(ref.shape))
        io = {"z": z.numel() * 4, "img": ref.size * 4}
        keep = (dec, p)
    np.savez(npz, **arrays)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0.05
    _BUILT[name] = dict(path=path, npz=npz, ref=ref, io=io, arrays=arrays, kind=kind, keep=keep)
    return _BUILT[name]


def _head(path):
    """(head region bytes, layout, file size) of a bundle file"""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        first = f.read(min(size, 64 << 20))
    lay = R.parse(first)
    return first[:lay.head], lay, size


@pytest.mark.parametrize("name", list(_CASES))
def test_real_bundle_passes_the_host_reader_and_runs_without_torch(name, workdir, driver):
    from stable_renderer_amd import _lib
    c = _case(name, workdir)
    # ---- the host-only reader accepts what the exporter writes, and validated every relocation with the extent computed here
    lines, _ = R.run_driver(driver, [c["path"]])
    _, rc, msg, ext = R.parse_report(lines[0])
    assert rc == 0, msg
    head, lay, _ = _head(c["path"])
    assert ext == R.expected_extents(head) and len(ext) == sum(p.n_rel for p in lay.plans) > 20
    kinds = {op.kind for p in lay.plans for op in p.ops}
    print(name, "ops", sum(p.n_ops for p in lay.plans), "relocations", len(ext), "kinds", sorted(kinds))
    # ---- a process without torch reproduces the Python plan bit for bit
    spec = dict(model=c["path"], kind=c["kind"], npz=c["npz"], out=str(workdir / (name + ".out.npz")), io=c["io"])
    (workdir / (name + ".json")).write_text(json.dumps(spec))
    child = workdir / "child2.py"
    child.write_text(CHILD2)
    r = subprocess.run([sys.executable, str(child), _lib.LIB_PATH, str(workdir / (name + ".json"))], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, PYTHONPATH=""))
    assert r.returncode == 0, r.stderr[-3000:]
    o = np.load(spec["out"])
    assert np.array_equal(o["out"], c["ref"]) and np.array_equal(o["out2"], c["ref"])


def test_bundles_cover_the_paths_they_are_meant_to(workdir):
    from stable_renderer_amd import _lib as L
    def ops(name):
        return [op for p in _head(_case(name, workdir)["path"])[1].plans for op in p.ops]
    assert any(op.kind == L.OP_IGEMM and op.u.igemm.up_h for op in ops("sd15_f16_odd"))                    # odd latent: up_h / up_w
    assert any(op.kind in (L.OP_GATHER_ROWS, L.OP_LAYERNORM_GATHER) for op in ops("sd15_f16_inject"))
    assert not any(op.kind in (L.OP_GATHER_ROWS, L.OP_LAYERNORM_GATHER) for op in ops("sd15_f32_plain"))
    assert "y" in _case("sdxl_f16_inject", workdir)["io"] and "y" not in _case("sd15_f16_inject", workdir)["io"]
    sm = [op.u.ew for op in ops("vae_f16_13x2") if op.kind == L.OP_SOFTMAX_ROWS]
    assert sm and all(e.cols > e.rows == 26 for e in sm)                                                   # padded keys


def test_groupnorm_scratch_restatement_equals_the_library():
    from stable_renderer_amd import _lib as L
    for b in (1, 2, 3, 4, 5, 7, 8, 9, 16, 33):
        for hw in (1, 63, 64, 65, 130, 4096, 4097, 16384, 65536):
            assert L.lib().sr_groupnorm_scratch_floats(b, hw) == R.gn_scratch_floats(b, hw), (b, hw)


def _load(path):
    from stable_renderer_amd import _lib as L
    h = C.c_void_p()
    rc = L.lib().sr_model_load(str(path).encode(), C.byref(h))
    return rc, h, L.lib().sr_last_error().decode()


def test_hostile_files_are_refused_by_sr_model_load_before_anything_runs(workdir):
    """every mutation of tests/bundle_ref.py applied to the head of the real tiny-UNet bundle: SR_ERR_INVALID, *out == NULL, the
    message names the reason.  Nothing here runs a plan: a file that loads is freed at once and fails the test."""
    from stable_renderer_amd import _lib as L
    c = _case("sd15_f16_inject", workdir)
    head, lay, size = _head(c["path"])
    total_mem = torch.cuda.mem_get_info()[1]
    muts = R.mutations(head, total_mem, file_size=size, first_only=True)
    names = [m[0] for m in muts]
    assert len(muts) > 60 and {"tensor:sum>limit", "tensor:sum_overflows", "reloc:offset=nbytes", "reloc:field_twice", "raw_address", "io:inject_err=0bytes",
                               "kind=16", "lane=2"} <= set(names)
    hostile = workdir / "hostile.srm"
    with open(c["path"], "rb") as src, open(hostile, "wb") as dst:
        while True:
            chunk = src.read(8 << 20)
            if not chunk:
                break
            dst.write(chunk)
    rc, h, msg = _load(hostile)                                 # the copy itself is sound
    assert rc == 0 and h.value, msg
    assert L.lib().sr_model_free(h) == 0
    bad = []
    for name, blob, phrases in muts:
        assert len(blob) == len(head)
        with open(hostile, "r+b") as f:
            f.write(blob)
        rc, h, msg = _load(hostile)
        if h.value:                                             # it loaded: free it, never run it
            L.lib().sr_model_free(h)
        if rc != R.INVALID or h.value or not any(p in msg for p in phrases):
            bad.append((name, rc, bool(h.value), msg))
    assert not bad, bad
    for cut in (lay.head - 1, lay.head // 2 // 8 * 8, 24, 8):   # truncated heads
        with open(hostile, "wb") as f:
            f.write(head[:cut])
        rc, h, msg = _load(hostile)
        if h.value:
            L.lib().sr_model_free(h)
        assert rc == R.INVALID and not h.value, (cut, msg)


def _forward(lib, h, arrays, ctx=True, stream=None):
    vp = C.c_void_p
    x, t, cx = (np.ascontiguousarray(arrays[k]) for k in ("x", "t", "ctx"))
    out = np.full_like(x, np.nan)
    rc = lib.sr_unet_forward(h, x.ctypes.data_as(vp), t.ctypes.data_as(vp), cx.ctypes.data_as(vp) if ctx else None, out.ctypes.data_as(vp), stream)
    return rc, out


def test_run_time_errors_and_the_inject_flag(workdir):
    from stable_renderer_amd import _lib as L
    lib, vp = L.lib(), C.c_void_p
    c = _case("sd15_f16_inject", workdir)
    B = c["arrays"]["x"].shape[0]
    rc, h, msg = _load(c["path"])
    assert rc == 0, msg
    try:
        for name, want in c["io"].items():                      # every window reports its size
            nb, ptr = C.c_int64(), vp()
            assert lib.sr_model_io(h, name.encode(), C.byref(ptr), C.byref(nb)) == 0 and nb.value == want and ptr.value, name
        assert set(c["io"]) == {"x", "t", "ctx", "out", "inject", "inject_err"}
        assert lib.sr_model_io(h, b"nope", None, None) == R.INVALID and "has no input / output named 'nope'" in lib.sr_last_error().decode()
        buf = np.zeros(4, np.int32)
        assert lib.sr_model_write(h, b"nope", buf.ctypes.data_as(vp), None) == R.INVALID
        assert lib.sr_model_read(h, b"nope", buf.ctypes.data_as(vp), None) == R.INVALID
        assert lib.sr_model_run(h, b"nope", None) == R.INVALID and "has no plan named 'nope'" in lib.sr_last_error().decode()
        # ctx == NULL before any prompt
        rc, _ = _forward(lib, h, c["arrays"], ctx=False)
        assert rc == R.INVALID and "there has been none" in lib.sr_last_error().decode()
        # an injected index outside the batch: zero-filled rows, the flag, SR_ERR_INVALID -- and the flag is cleared for the next call
        inj = np.array([B], np.int32)
        assert lib.sr_model_write(h, b"inject", inj.ctypes.data_as(vp), None) == 0
        rc, _ = _forward(lib, h, c["arrays"])
        assert rc == R.INVALID and "lies outside the batch" in lib.sr_last_error().decode()
        inj = np.ascontiguousarray(c["arrays"]["inject"])
        assert lib.sr_model_write(h, b"inject", inj.ctypes.data_as(vp), None) == 0
        rc, out = _forward(lib, h, c["arrays"])
        assert rc == 0, lib.sr_last_error().decode()
        assert lib.sr_device_sync() == 0 and np.array_equal(out, c["ref"])
        rc, out = _forward(lib, h, c["arrays"], ctx=False)       # same prompt again
        assert rc == 0 and lib.sr_device_sync() == 0 and np.array_equal(out, c["ref"])
    finally:
        assert lib.sr_model_free(h) == 0
    assert lib.sr_model_free(None) == 0


def test_a_callers_stream_and_two_models_alive(workdir):
    from stable_renderer_amd import _lib as L
    lib, vp = L.lib(), C.c_void_p
    cu, cv = _case("sd15_f32_plain", workdir), _case("vae_f16_13x2", workdir)
    rc, hu, msg = _load(cu["path"])
    assert rc == 0, msg
    rc, hv, msg = _load(cv["path"])
    assert rc == 0, msg
    try:
        z = np.ascontiguousarray(cv["arrays"]["z"])
        for _ in range(2):                                      # alternately, each its own bits
            rc, out = _forward(lib, hu, cu["arrays"])
            assert rc == 0, lib.sr_last_error().decode()
            img = np.full(cv["ref"].shape, np.nan, np.float32)
            assert lib.sr_vae_decode(hv, z.ctypes.data_as(vp), img.ctypes.data_as(vp), None) == 0, lib.sr_last_error().decode()
            assert lib.sr_device_sync() == 0
            assert np.array_equal(out, cu["ref"]) and np.array_equal(img, cv["ref"])
        s = torch.cuda.Stream()
        rc, out = _forward(lib, hu, cu["arrays"], stream=vp(s.cuda_stream))
        assert rc == 0, lib.sr_last_error().decode()
        img = np.full(cv["ref"].shape, np.nan, np.float32)
        assert lib.sr_vae_decode(hv, z.ctypes.data_as(vp), img.ctypes.data_as(vp), vp(s.cuda_stream)) == 0
        s.synchronize()
        assert np.array_equal(out, cu["ref"]) and np.array_equal(img, cv["ref"])
    finally:
        assert lib.sr_model_free(hu) == 0 and lib.sr_model_free(hv) == 0
