"""The poisoned-arena harness (tests/arena.py) through the C ABI of the rasteriser and the side libraries (resample, tiled,
imgproc, morph): every call runs on ordinary torch tensors and again with its outputs, temporaries and scratch carved out of one
arena at exactly the documented sizes, 16 bytes past a 256-byte boundary, between NaN guards.  Equal return codes, equal bits,
no byte touched outside the operands.  (esrgan carries its own guard bands: tests/test_gpu_esrgan.py.)"""
import ctypes as C

import pytest
import torch

import arena as A

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, I32, I64, F64, U8 = torch.float32, torch.float16, torch.int32, torch.int64, torch.float64, torch.uint8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stable_renderer_amd import ops as o
    return o


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def i64x(*v):
    return (C.c_int64 * len(v))(*v)


def poisoned(dtype, *shape):
    """a plain output: filled, so that an element the call does not write differs from anything it could write"""
    t = torch.empty(*shape, dtype=dtype, device=DEV)
    bits(t.view(-1)).fill_(A.POISON[t.element_size()] if t.element_size() < 8 else 0x5A5A5A5A5A5A5A5A)
    return t


def both(call, ins=None, outs=None, scratch=None, inout=None, expect=0):
    """call(P) -> return code, P: name -> device address.  ins / inout: name -> tensor; outs: name -> (dtype, rows, cols) with the
    rows an image row or a plane; scratch: name -> (bytes, dtype).  Runs plain, then in one arena; -> the arena"""
    ins, outs, scratch, inout = ins or {}, outs or {}, scratch or {}, inout or {}
    keep, ar = {}, A.Arena(DEV)
    for n, t in ins.items():
        keep[n] = t.contiguous().clone()
        ar.input(n, t, pitch_bytes=t.stride(-2) * t.element_size() if t.dim() > 1 else 0)
    for n, (dt, rows, cols) in outs.items():
        keep[n] = poisoned(dt, rows, cols)
        ar.output(n, dt, rows, cols)
    for n, (nbytes, dt) in scratch.items():
        keep[n] = torch.empty(2 * nbytes + 4096, dtype=U8, device=DEV)
        ar.scratch(n, nbytes, dt)
    for n, t in inout.items():
        keep[n] = t.contiguous().clone()
        ar.inout(n, t, pitch_bytes=t.stride(-2) * t.element_size() if t.dim() > 1 else 0)
    ar.build()
    assert ar.address_ok()
    rc_p = call({n: t.data_ptr() for n, t in keep.items()})
    rc_a = call({n: ar.ptr(n) for n in keep})
    torch.cuda.synchronize()
    assert rc_p == rc_a == expect, (rc_p, rc_a)
    if rc_a == 0:
        for n in outs:
            assert torch.equal(bits(keep[n]), bits(ar.result(n))), f"output '{n}' differs between the plain and the arena form"
        for n in inout:
            assert torch.equal(bits(keep[n].view(-1)), bits(ar.view(n))), f"'{n}' differs between the plain and the arena form"
    for n, t in ins.items():
        assert torch.equal(bits(keep[n]), bits(t.contiguous())), f"plain input '{n}' modified"
    report = ar.check()
    assert report == [], "\n".join(report)
    return ar


def view_extent(x):
    """a strided view as the library receives it: (its base's memory cut after the view's last element, the view's element offset)"""
    off = x.storage_offset()
    last = off + sum((n - 1) * st for n, st in zip(x.shape, x.stride())) + 1
    base = x._base if x._base is not None else x
    assert base.is_contiguous() and base.storage_offset() == 0
    return base.reshape(-1)[:last].to(DEV), off


# ---- rasteriser -------------------------------------------------------------------------------------------------------------

PLANES = [("color", F16, 4), ("id", I32, 4), ("pos", F32, 3), ("normal_depth", F16, 4), ("noise", F16, 4), ("canny", F32, 3),
          ("zbuf", F32, 1)]


def arena_gbuffer(S, L, ar, prefix, W, H):
    """a scene.GBuffer whose seven planes are sub-buffers of the arena"""
    g = S.GBuffer.__new__(S.GBuffer)
    g.W, g.H, g._scratch = W, H, None
    c = L.GBuffer()
    for name, dt, comps in PLANES:
        v = ar.view(prefix + name)
        setattr(g, name, v.view(H, W, comps) if comps > 1 else v.view(H, W))
        setattr(c, name, ar.ptr(prefix + name))
    c.W, c.H = W, H
    g.c = c
    return g


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33), (200, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_raster_planes_and_scratch(ops, size):
    """clear, three draws (vertex colours, textured + noise, baking with texcoord ids), the identical-G-buffer merge and the
    display pass: all seven planes of both G-buffers, each draw's scratch at exactly sr_raster_scratch_bytes, the display image"""
    from stable_renderer_amd import scene as S
    from test_gpu_raster import _scene
    L = ops.L
    lib = L.lib()
    W, H = size
    cam, tasks = _scene(W, H, 5)
    tasks = sorted(tasks, key=lambda t: t.order)
    view, proj = cam.view(), cam.projection(W / H)
    needs = [lib.sr_raster_scratch_bytes(t.mesh.tris.shape[0], W, H) for t in tasks]
    assert min(needs) > 0

    ar = A.Arena(DEV)
    for prefix in ("acc.", "tmp."):
        for name, dt, comps in PLANES:
            ar.output(prefix + name, dt, H, W * comps)
    for i, need in enumerate(needs):
        ar.scratch(f"scratch{i}", need, F32 if need % 4 == 0 else U8)
    ar.output("display", F32, H, W * 4)
    ar.build()
    assert ar.address_ok()

    def run(acc, tmp, scratches, display_ptr):
        """ordinary render into tmp; then every task alone into tmp, merged into acc by depth; then acc's display image"""
        snap = []
        tmp.clear()
        for t, s in zip(tasks, scratches):
            tmp._scratch = s
            tmp.draw(t, view, proj)
        torch.cuda.synchronize()
        snap += [getattr(tmp, n).clone() for n, _, _ in PLANES]
        acc.clear()
        for t, s in zip(tasks, scratches):
            tmp.clear()
            tmp._scratch = s
            tmp.draw(t, view, proj)
            L.check(lib.sr_gbuffer_depth_merge(C.byref(acc.c), C.byref(tmp.c), ops.stream_ptr()))
        L.check(lib.sr_defer_post(acc.color.data_ptr(), acc.id.data_ptr(), display_ptr, W, H, 1, 1, 1, 2.2, 1.1, 0.9, 1.05, 1.1,
                                  ops.stream_ptr()))
        torch.cuda.synchronize()
        return snap + [getattr(g, n).clone() for g in (acc, tmp) for n, _, _ in PLANES]

    disp = poisoned(F32, H, W * 4)
    plain = run(S.GBuffer(W, H), S.GBuffer(W, H), [torch.empty(n + 4096, dtype=U8, device=DEV) for n in needs], disp.data_ptr())
    scr = [ar.view(f"scratch{i}").view(U8)[:n] for i, n in enumerate(needs)]
    assert all(s.numel() == n and s.data_ptr() == ar.ptr(f"scratch{i}") for i, (s, n) in enumerate(zip(scr, needs)))
    inside = run(arena_gbuffer(S, L, ar, "acc.", W, H), arena_gbuffer(S, L, ar, "tmp.", W, H), scr, ar.ptr("display"))
    for i, (a, b) in enumerate(zip(plain, inside)):
        assert torch.equal(bits(a), bits(b)), f"plane {PLANES[i % 7][0]} of stage {i // 7} differs between the plain and the arena form"
    assert torch.equal(bits(disp), bits(ar.result("display")))
    assert int((plain[1][..., 0] != 0).sum()) > 0 or W * H == 1              # the scene covers pixels
    report = ar.check()
    assert report == [], "\n".join(report)


# ---- resample ---------------------------------------------------------------------------------------------------------------

RESIZES = [((13, 17), (29, 11)), ((9, 7), (4, 15)), ((5, 6), (5, 13)), ((1, 1), (3, 2))]


@pytest.mark.parametrize("mode", ["nearest-exact", "nearest", "bilinear", "bicubic", "area"])
def test_resample_modes(ops, mode):
    from stable_renderer_amd import resample as RS
    from stable_renderer_amd import _lib_resample as LR
    g = torch.Generator().manual_seed(2)
    for (Hi, Wi), (Ho, Wo) in RESIZES:
        N, Cc = 2, 3
        x = torch.randn(N, Cc, Hi, Wi, generator=g).to(DEV)
        both(lambda P: LR.lib().sr_resample(P["src"], P["dst"], N, Cc, Hi, Wi, Ho, Wo, i64x(*x.stride()),
                                            i64x(Cc * Ho * Wo, Ho * Wo, Wo, 1), RS.MODES[mode], ops.stream_ptr()),
             ins={"src": x}, outs={"dst": (F32, N * Cc * Ho, Wo)})
        # an IMAGE resampled where it lies (image.movedim(-1, 1)), into NHWC memory
        v = torch.randn(N, Hi, Wi, Cc, generator=g).movedim(-1, 1)
        base, off = view_extent(v)
        both(lambda P: LR.lib().sr_resample(P["src"] + 4 * off, P["dst"], N, Cc, Hi, Wi, Ho, Wo, i64x(*v.stride()),
                                            i64x(Ho * Wo * Cc, 1, Wo * Cc, Cc), RS.MODES[mode], ops.stream_ptr()),
             ins={"src": base}, outs={"dst": (F32, N * Ho, Wo * Cc)})
        # a centre crop: a pointer offset into a larger tensor that ends at the crop's last element
        v = torch.randn(N, Cc, Hi + 4, Wi + 6, generator=g)[:, :, 2:2 + Hi, 3:3 + Wi]
        base, off = view_extent(v)
        both(lambda P: LR.lib().sr_resample(P["src"] + 4 * off, P["dst"], N, Cc, Hi, Wi, Ho, Wo, i64x(*v.stride()),
                                            i64x(Cc * Ho * Wo, Ho * Wo, Wo, 1), RS.MODES[mode], ops.stream_ptr()),
             ins={"src": base}, outs={"dst": (F32, N * Cc * Ho, Wo)})


def test_bislerp_with_its_temporary_at_exact_size(ops):
    from stable_renderer_amd import resample as RS
    from stable_renderer_amd import _lib_resample as LR
    g = torch.Generator().manual_seed(3)
    for (Hi, Wi), (Ho, Wo) in RESIZES:
        N, Cc = 2, 4
        x = torch.randn(N, Cc, Hi, Wi, generator=g).to(DEV)
        xt = [torch.from_numpy(a).to(DEV) for a in RS.bilinear_tables(Wi, Wo)]
        yt = [torch.from_numpy(a).to(DEV) for a in RS.bilinear_tables(Hi, Ho)]
        assert all(t.numel() == Wo for t in xt) and all(t.numel() == Ho for t in yt)
        both(lambda P: LR.lib().sr_bislerp(P["src"], P["dst"], P["tmp"], N, Cc, Hi, Wi, Ho, Wo, i64x(*x.stride()), P["xr"], P["x1"], P["x2"],
                                           P["yr"], P["y1"], P["y2"], ops.stream_ptr()),
             ins={"src": x, "xr": xt[0], "x1": xt[1], "x2": xt[2], "yr": yt[0], "y1": yt[1], "y2": yt[2]},
             outs={"dst": (F32, N * Cc * Ho, Wo)}, scratch={"tmp": (N * Cc * Hi * Wo * 8, F64)})


def test_lanczos_with_its_temporary_at_exact_size(ops):
    from stable_renderer_amd import resample as RS
    from stable_renderer_amd import _lib_resample as LR
    g = torch.Generator().manual_seed(4)
    for (Hi, Wi), (Ho, Wo) in RESIZES[:2] + [((9, 7), (9, 12)), ((9, 7), (5, 7))]:
        N = 2
        x = torch.rand(N, 3, Hi, Wi, generator=g).to(DEV)
        ins, sc = {"src": x}, {}
        xks = yks = 0
        if Wi != Wo:
            b, k, xks = RS.lanczos_taps(Wi, Wo)
            ins["xb"], ins["xk"] = torch.from_numpy(b).to(DEV), torch.from_numpy(k).to(DEV)
        if Hi != Ho:
            b, k, yks = RS.lanczos_taps(Hi, Ho)
            ins["yb"], ins["yk"] = torch.from_numpy(b).to(DEV), torch.from_numpy(k).to(DEV)
        if Wi != Wo and Hi != Ho:
            sc["tmp"] = (N * Hi * Wo * 3, U8)
        both(lambda P: LR.lib().sr_lanczos_rgb8(P["src"], P["dst"], P.get("tmp"), N, Hi, Wi, Ho, Wo, i64x(*x.stride()),
                                                i64x(3 * Ho * Wo, Ho * Wo, Wo, 1), P.get("xb"), P.get("xk"), xks, P.get("yb"), P.get("yk"),
                                                yks, ops.stream_ptr()),
             ins=ins, outs={"dst": (F32, N * 3 * Ho, Wo)}, scratch=sc)


# ---- tiled VAE helpers ------------------------------------------------------------------------------------------------------

def test_tile_gather_accumulate_finish_with_windows_on_every_border(ops):
    from stable_renderer_amd import _lib_tiled as LT
    lib = LT.lib()
    g = torch.Generator().manual_seed(5)
    planes, H, W, th, tw, feather = 3, 19, 23, 8, 10, 3
    windows = [(0, 0), (0, W - tw), (H - th, 0), (H - th, W - tw), (5, 6), (0, 7), (H - th, 7), (4, 0), (4, W - tw)]
    src = torch.randn(planes, H, W, generator=g).to(DEV)
    for y0, x0 in windows:
        both(lambda P: lib.sr_tile_gather(P["src"], P["dst"], planes, H, W, y0, x0, th, tw, ops.stream_ptr()),
             ins={"src": src}, outs={"dst": (F32, planes * th, tw)})
    both(lambda P: lib.sr_tile_gather(P["src"], P["dst"], planes, H, W, 0, 0, H, W, ops.stream_ptr()),
         ins={"src": src}, outs={"dst": (F32, planes * H, W)})
    for cpp, npl in ((1, 3), (3, 2)):
        accs, wsums = [], []
        for k in range(3):
            acc = torch.zeros(npl, H, W * cpp, device=DEV)
            wsum = torch.zeros(H, W, dtype=I64, device=DEV)
            for y0, x0 in windows:
                tile = torch.randn(npl, th, tw * cpp, generator=g).to(DEV)
                ar = both(lambda P: lib.sr_tile_accumulate(P["tile"], P["acc"], P["wsum"], npl, H, W, cpp, y0, x0, th, tw, feather,
                                                           ops.stream_ptr()),
                          ins={"tile": tile}, inout={"acc": acc, "wsum": wsum})
                acc, wsum = ar.view("acc").view(npl, H, W * cpp).clone(), ar.view("wsum").view(H, W).clone()
            accs.append(acc)
            wsums.append(wsum)
        assert int(wsums[0].min()) > 0                          # the windows cover the image
        for npass in (1, 2, 3):
            for mode in (0, 1):
                ins = {f"acc{k}": accs[k] for k in range(npass)}
                ins.update({f"wsum{k}": wsums[k] for k in range(npass)})
                both(lambda P: lib.sr_tile_finish(P["acc0"], P.get("acc1"), P.get("acc2"), P["wsum0"], P.get("wsum1"), P.get("wsum2"),
                                                  P["out"], npl, H, W, cpp, npass, feather, mode, ops.stream_ptr()),
                     ins=ins, outs={"out": (F32, npl * H, W * cpp)})


def test_softmax_rows_ld_in_place(ops):
    from stable_renderer_amd import _lib_tiled as LT
    g = torch.Generator().manual_seed(6)
    for dt, code in ((F16, 0), (F32, 1)):
        for rows, cols, ld in ((5, 37, 40), (3, 300, 304), (2, 8, 8)):
            x = (torch.randn(rows, ld, generator=g) * 3).to(dt).to(DEV)
            both(lambda P: LT.lib().sr_softmax_rows_ld(P["x"], rows, cols, ld, code, ops.stream_ptr()), inout={"x": x})


# ---- imgproc ----------------------------------------------------------------------------------------------------------------

def test_imgproc_entry_points(ops):
    from stable_renderer_amd import _lib_imgproc as LI
    lib = LI.lib()
    st = ops.stream_ptr
    g = torch.Generator().manual_seed(7)
    B, H, W, Cc = 2, 37, 21, 3
    img = torch.rand(B, H, W, Cc, generator=g).to(DEV)
    img2 = torch.rand(B, H, W, Cc, generator=g).to(DEV)
    for radius, amount in ((1, 0.0), (3, 0.0), (5, 0.7), (20, 0.0)):
        both(lambda P: lib.sr_filter_gauss(P["src"], P["dst"], B, H, W, Cc, i64x(*img.stride()), radius, 1.3, amount, st()),
             ins={"src": img}, outs={"dst": (F32, B * H, W * Cc)})
    import imgproc_ref as IR
    for i, (shape, radius, sigma) in enumerate(IR.GAUSS_CASES):              # the cases of test_gpu_imgproc.py (r = 31 among them)
        x = IR.gauss_input(i)
        b_, h_, w_, c_ = x.shape
        # the strided view stays one: its base tensor, cut after the view's last element, and a pointer offset into it
        base, off = view_extent(x)
        assert (i == IR.GAUSS_VIEW) == (not x.is_contiguous())
        for amount in (0.0, 10 * IR.SHARPEN_ALPHAS[0]):
            both(lambda P: lib.sr_filter_gauss(P["src"] + 4 * off, P["dst"], b_, h_, w_, c_, i64x(*x.stride()), radius, sigma, amount, st()),
                 ins={"src": base}, outs={"dst": (F32, b_ * h_, w_ * c_)})
    for shape, expand, tapered in IR.GROW_CASES:
        m = IR.grow_input(shape).to(DEV)
        n_, h_, w_ = shape
        need_tmp = min(abs(expand), h_ + w_) > 16                              # SR_GROW_MAX_STEP
        both(lambda P: lib.sr_mask_grow(P["src"], P["dst"], P.get("tmp"), n_, h_, w_, i64x(*m.stride()), expand, int(tapered), st()),
             ins={"src": m}, outs={"dst": (F32, n_ * h_, w_)}, scratch={"tmp": (n_ * h_ * w_ * 4, F32)} if need_tmp else None)
    mask = (torch.rand(B, H, W, generator=g) > 0.7).float().to(DEV) * torch.rand(B, H, W, generator=g).to(DEV)
    for expand, tapered in ((0, 0), (1, 1), (3, 0), (-2, 1), (16, 1)):         # one launch: no temporary
        both(lambda P: lib.sr_mask_grow(P["src"], P["dst"], None, B, H, W, i64x(*mask.stride()), expand, tapered, st()),
             ins={"src": mask}, outs={"dst": (F32, B * H, W)})
    for expand, tapered in ((17, 1), (-20, 0), (40, 0), (100, 1)):            # several launches through tmp (N, H, W) at exact size
        both(lambda P: lib.sr_mask_grow(P["src"], P["dst"], P["tmp"], B, H, W, i64x(*mask.stride()), expand, tapered, st()),
             ins={"src": mask}, outs={"dst": (F32, B * H, W)}, scratch={"tmp": (B * H * W * 4, F32)})
    for l, t, r, b in ((3, 0, 0, 5), (0, 4, 6, 0), (50, 50, 50, 50), (1, 1, 1, 1)):
        both(lambda P: lib.sr_mask_feather(P["src"], P["dst"], B, H, W, i64x(*mask.stride()), l, t, r, b, st()),
             ins={"src": mask}, outs={"dst": (F32, B * H, W)})
    for mode in range(6):
        both(lambda P: lib.sr_blend(P["a"], P["b"], P["dst"], B, H, W, Cc, i64x(*img.stride()), i64x(*img2.stride()), 0.35, mode, st()),
             ins={"a": img, "b": img2}, outs={"dst": (F32, B * H, W * Cc)})
    # composite: an NCHW destination, a source placed against each border, with and without a mask
    dst = torch.rand(B, Cc, H, W, generator=g).to(DEV)
    hs, ws = 9, 8
    srcc = torch.rand(1, Cc, hs, ws, generator=g).to(DEV)
    cm = torch.rand(B, hs, ws, generator=g).to(DEV)
    for top, left in ((0, 0), (H - hs, W - ws), (0, W - ws), (H - hs, 0), (11, 5)):
        for use_mask in (False, True):
            both(lambda P: lib.sr_composite(P["dst"], P["src"], P.get("mask"), B, Cc, H, W, 1, B, top, left, hs, ws, i64x(*dst.stride()),
                                            i64x(*srcc.stride()), i64x(*cm.stride()) if use_mask else None, st()),
                 ins={"src": srcc, **({"mask": cm} if use_mask else {})}, inout={"dst": dst})
    srcm = torch.rand(1, 10, 30, generator=g).to(DEV)
    for op in range(6):
        for x, y in ((0, 0), (15, 30), (W - 1, H - 1)):
            both(lambda P: lib.sr_mask_combine(P["dest"], P["source"], P["dst"], B, H, W, 1, 10, 30, i64x(*mask.stride()),
                                               i64x(*srcm.stride()), x, y, op, st()),
                 ins={"dest": mask, "source": srcm}, outs={"dst": (F32, B * H, W)})
    q = (torch.randint(0, 3, (B, H, W, Cc), generator=g).float() / 2).to(DEV)
    both(lambda P: lib.sr_color_to_mask(P["image"], P["dst"], B, H, W, i64x(*q.stride()), 0xFF8000, st()),
         ins={"image": q}, outs={"dst": (F32, B * H, W)})


# ---- morph ------------------------------------------------------------------------------------------------------------------

def test_morph_box_with_scratch_at_exactly_the_required_count(ops):
    from stable_renderer_amd import _morph as LM
    lib = LM.lib()
    g = torch.Generator().manual_seed(8)
    for shape in ((2, 13, 9, 3), (1, 70, 37, 1), (1, 1, 1, 4)):
        B, H, W, Cc = shape
        n = B * H * W * Cc
        x = torch.rand(*shape, generator=g).to(DEV)
        e = torch.rand(*shape, generator=g).to(DEV)
        for k in (1, 2, 3, 8, 65):
            both(lambda P: lib.sr_morph_box(P["src"], P["mx"], P["mn"], P["scratch"], 2 * n, B, H, W, Cc, i64x(*x.stride()), k, 0, None,
                                            None, ops.stream_ptr()),
                 ins={"src": x}, outs={"mx": (F32, B * H, W * Cc), "mn": (F32, B * H, W * Cc)}, scratch={"scratch": (2 * n * 4, F32)})
            both(lambda P: lib.sr_morph_box(P["src"], P["mx"], None, P["scratch"], n, B, H, W, Cc, i64x(*x.stride()), k, 0, None, None,
                                            ops.stream_ptr()),
                 ins={"src": x}, outs={"mx": (F32, B * H, W * Cc)}, scratch={"scratch": (n * 4, F32)})
            both(lambda P: lib.sr_morph_box(P["src"], None, P["mn"], P["scratch"], n, B, H, W, Cc, i64x(*x.stride()), k, 3, P["epi"],
                                            i64x(*e.stride()), ops.stream_ptr()),
                 ins={"src": x, "epi": e}, outs={"mn": (F32, B * H, W * Cc)}, scratch={"scratch": (n * 4, F32)})
            both(lambda P: lib.sr_morph_box(P["src"], P["mx"], None, P["scratch"], 2 * n, B, H, W, Cc, i64x(*x.stride()), k, 1, None, None,
                                            ops.stream_ptr()),
                 ins={"src": x}, outs={"mx": (F32, B * H, W * Cc)}, scratch={"scratch": (2 * n * 4, F32)})
        # one float short is refused, nothing is touched
        both(lambda P: lib.sr_morph_box(P["src"], P["mx"], P["mn"], P["scratch"], 2 * n - 1, B, H, W, Cc, i64x(*x.stride()), 3, 0, None,
                                        None, ops.stream_ptr()),
             ins={"src": x}, outs={"mx": (F32, B * H, W * Cc), "mn": (F32, B * H, W * Cc)}, scratch={"scratch": (2 * n * 4, F32)},
             expect=-1)


def test_porter_duff_every_mode(ops):
    from stable_renderer_amd import _morph as LM
    lib = LM.lib()
    g = torch.Generator().manual_seed(9)
    n_pix, Cc = 1237, 3
    s, d = torch.rand(n_pix, Cc, generator=g).to(DEV), torch.rand(n_pix, Cc, generator=g).to(DEV)
    sa, da = torch.rand(n_pix, generator=g).to(DEV), torch.rand(n_pix, generator=g).to(DEV)
    for mode in range(18):
        both(lambda P: lib.sr_porter_duff(P["s"], P["sa"], P["d"], P["da"], P["oi"], P["oa"], n_pix, Cc, mode, ops.stream_ptr()),
             ins={"s": s, "sa": sa, "d": d, "da": da}, outs={"oi": (F32, 1, n_pix * Cc), "oa": (F32, 1, n_pix)})
