"""ctypes binding of libsr_hip.so (C ABI in include/sr_hip.h).  The product path has NO CPU fallback: if
the shared library is missing or a symbol is absent, import of the compute modules fails loudly."""
import ctypes as C
import os

from . import _native
from ._native import SrHipError  # noqa: F401  (raised by every loader; its users import it from here)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libsr_hip.so")
_DEV_LIB = os.environ.get("SR_DEV_LIB")          # development only: an experimental build of the library (tools/); no hash check

SR_F16, SR_F32 = 0, 1
(OP_IGEMM, OP_GROUPNORM, OP_LAYERNORM, OP_ATTENTION, OP_NCHW_TO_NHWC, OP_NHWC_TO_NCHW, OP_TIMESTEP_EMBED, OP_SILU,
 OP_SOFTMAX_ROWS, OP_GATHER_ROWS, OP_ADD_SCALED, OP_FORK, OP_JOIN, OP_ROW_STATS, OP_LAYERNORM_GATHER) = range(1, 16)

vp = C.c_void_p
i32 = C.c_int32
i64 = C.c_int64
f32 = C.c_float


class IgemmArgs(C.Structure):
    _fields_ = [("a", vp), ("a2", vp), ("w", vp), ("bias", vp), ("rowvec", vp), ("residual", vp), ("out", vp),
                ("zero_page", vp), ("B", i32), ("H", i32), ("W", i32), ("C1", i32), ("C2", i32), ("N", i32),
                ("KH", i32), ("stride", i32), ("upsample", i32), ("act", i32), ("transpose_out", i32), ("ldt", i32),
                ("out_f32", i32), ("dtype", i32), ("scale", f32), ("rowvec_ld", i32), ("workspace", vp),
                ("workspace_bytes", C.c_int64), ("row_stats", vp), ("colsum", vp), ("tile", i32), ("split", i32), ("pad_br", i32),
                ("prefetch", vp), ("prefetch_bytes", C.c_int64), ("up_h", i32), ("up_w", i32), ("split_counters", vp), ("group", i32), ("ln_inline", i32), ("ln_eps", f32), ("tile_order", i32)]


class GroupNormArgs(C.Structure):
    _fields_ = [("x", vp), ("x2", vp), ("gamma", vp), ("beta", vp), ("y", vp), ("partials", vp), ("B", i32),
                ("HW", i32), ("C1", i32), ("C2", i32), ("groups", i32), ("silu", i32), ("dtype", i32), ("eps", f32)]


class AttentionArgs(C.Structure):
    _fields_ = [("q", vp), ("k", vp), ("vt", vp), ("o", vp), ("B", i32), ("Bk", i32), ("Tq", i32), ("Tk", i32),
                ("heads", i32), ("d", i32), ("ldt", i32), ("dtype", i32), ("q_stride", i32), ("k_stride", i32),
                ("scale", f32)]


class _Ln(C.Structure):
    _fields_ = [("x", vp), ("gamma", vp), ("beta", vp), ("y", vp), ("rows", i32), ("C", i32), ("dtype", i32), ("eps", f32),
                ("sel", vp), ("err_flag", vp), ("frame_rows", i32), ("n_frames", i32)]


class _Cvt(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("per_batch_scale", vp), ("B", i32), ("C", i32), ("HW", i32), ("Cpad", i32),
                ("dtype", i32), ("ldc", i32), ("scale", f32)]


class _Temb(C.Structure):
    _fields_ = [("t", vp), ("y", vp), ("B", i32), ("dim", i32), ("dtype", i32)]


class _Ew(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("n", i64), ("dtype", i32), ("rows", i32), ("cols", i32)]


class _Gather(C.Structure):
    _fields_ = [("x", vp), ("y", vp), ("sel", vp), ("row_bytes", i64), ("nsel", i32), ("n_rows", i32), ("err_flag", vp)]


class _Add(C.Structure):
    _fields_ = [("a", vp), ("b", vp), ("y", vp), ("n", i64), ("s", f32), ("dtype", i32)]


class _OpU(C.Union):
    _fields_ = [("igemm", IgemmArgs), ("gn", GroupNormArgs), ("attn", AttentionArgs), ("ln", _Ln), ("cvt", _Cvt),
                ("temb", _Temb), ("ew", _Ew), ("gather", _Gather), ("add", _Add)]


class Op(C.Structure):
    _fields_ = [("kind", i32), ("lane", i32), ("u", _OpU)]


class Draw(C.Structure):
    _fields_ = [("pos", vp), ("normal", vp), ("uv", vp), ("color", vp), ("vertex_id", vp), ("tris", vp), ("nv", i32),
                ("nt", i32), ("MV", f32 * 16), ("MV_IT", f32 * 16), ("P", f32 * 16), ("sprite_id", i32),
                ("material_id", i32), ("corrmap_k", i32), ("use_texcoord_id", i32), ("render_mode", i32),
                ("has_vertex_color", i32), ("depth_test", i32), ("cull_back", i32), ("id_w", i32), ("id_h", i32),
                ("noise_tex", vp), ("noise_w", i32), ("noise_h", i32), ("diffuse_tex", vp), ("diffuse_w", i32),
                ("diffuse_h", i32), ("corrmap_tex", vp), ("corr_w", i32), ("corr_h", i32),
                ("tangent", vp), ("bitangent", vp), ("normal_tex", vp), ("normal_w", i32), ("normal_h", i32), ("diffuse_levels", i32)]


class GBuffer(C.Structure):
    _fields_ = [("color", vp), ("id", vp), ("pos", vp), ("normal_depth", vp), ("noise", vp), ("canny", vp), ("zbuf", vp),
                ("W", i32), ("H", i32)]


# every exported symbol of include/sr_hip.h: name -> (restype, argtypes)
P = C.POINTER
SYMBOLS = {
    "sr_last_error": (C.c_char_p, []),
    "sr_version": (C.c_int, []),
    "sr_source_hash": (C.c_char_p, []),
    "sr_device_sync": (C.c_int, []),
    "sr_model_load": (C.c_int, [C.c_char_p, P(vp)]),
    "sr_model_free": (C.c_int, [vp]),
    "sr_model_io": (C.c_int, [vp, C.c_char_p, P(vp), P(i64)]),
    "sr_model_run": (C.c_int, [vp, C.c_char_p, vp]),
    "sr_model_write": (C.c_int, [vp, C.c_char_p, vp, vp]),
    "sr_model_read": (C.c_int, [vp, C.c_char_p, vp, vp]),
    "sr_unet_forward": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "sr_vae_decode": (C.c_int, [vp, vp, vp, vp]),
    "sr_layernorm_gather": (C.c_int, [vp, vp, i32, i32, i32, vp, vp, vp, vp, i32, f32, i32, vp]),
    "sr_igemm": (C.c_int, [P(IgemmArgs), vp]),
    "sr_igemm_group": (C.c_int, [P(P(IgemmArgs)), i32, vp]),
    "sr_groupnorm": (C.c_int, [P(GroupNormArgs), vp]),
    "sr_groupnorm_scratch_floats": (i64, [i32, i32]),
    "sr_layernorm": (C.c_int, [vp, vp, vp, vp, i32, i32, f32, i32, vp]),
    "sr_row_stats": (C.c_int, [vp, vp, i32, i32, f32, i32, vp]),
    "sr_attention": (C.c_int, [P(AttentionArgs), vp]),
    "sr_nchw_to_nhwc": (C.c_int, [vp, vp, i32, i32, i32, i32, f32, vp, i32, vp]),
    "sr_nhwc_to_nchw": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "sr_timestep_embedding": (C.c_int, [vp, vp, i32, i32, i32, vp]),
    "sr_silu": (C.c_int, [vp, vp, i64, i32, vp]),
    "sr_cast": (C.c_int, [vp, i32, vp, i32, i64, vp]),
    "sr_cache_touch": (C.c_int, [vp, i64, vp]),
    "sr_softmax_rows": (C.c_int, [vp, i32, i32, i32, vp]),
    "sr_gather_rows": (C.c_int, [vp, vp, vp, i32, i32, i64, vp, vp]),
    "sr_add_scaled": (C.c_int, [vp, vp, vp, i64, f32, i32, vp]),
    "sr_plan_run": (C.c_int, [P(Op), i32, vp]),
    "sr_plan_capture": (C.c_int, [P(Op), i32, vp, P(vp)]),
    "sr_graph_launch": (C.c_int, [vp, vp]),
    "sr_graph_destroy": (C.c_int, [vp]),
    "sr_eps_scale_input": (C.c_int, [vp, vp, i64, i32, f32, vp]),
    "sr_cfg_denoise": (C.c_int, [vp, vp, vp, vp, i64, i32, f32, f32, vp]),
    "sr_cond_crop_scale": (C.c_int, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "sr_cond_accumulate": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, f32, vp]),
    "sr_cfg_combine": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, f32, f32, vp]),
    "sr_euler_step": (C.c_int, [vp, vp, i64, f32, vp]),
    "sr_vae_sample": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "sr_ddpm_step": (C.c_int, [vp, vp, vp, i64, f32, f32, vp]),
    "sr_lcm_step": (C.c_int, [vp, vp, vp, i64, f32, vp]),
    "sr_axpby": (C.c_int, [vp, vp, i64, f32, f32, vp]),
    "sr_idmap_masks": (C.c_int, [vp, vp, i64, vp]),
    "sr_overlap_build": (C.c_int, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]),
    "sr_overlap_csr_scratch_ints": (i64, [i32]),
    "sr_overlap_csr": (C.c_int, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "sr_overlap_step": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp]),
    "sr_legacy_overlap": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f32, i32, i32, i32, vp]),
    "sr_legacy_levels": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "sr_legacy_overlap_seq": (C.c_int, [vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, vp]),
    "sr_nearest_resize": (C.c_int, [vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    "sr_adain": (C.c_int, [vp, i64, i64, i64, i32, vp, i32, i64, i64, i64, i32, vp, i32, i32, f32, vp, vp]),
    "sr_noise_pool": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, vp, vp]),
    "sr_noise_pool_strips": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "sr_corrmap_update": (C.c_int, [vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, vp]),
    "sr_gbuffer_clear": (C.c_int, [P(GBuffer), vp]),
    "sr_gbuffer_depth_merge": (C.c_int, [P(GBuffer), P(GBuffer), vp]),
    "sr_defer_post": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, f32, f32, f32, vp]),
    "sr_raster_draw": (C.c_int, [P(Draw), P(GBuffer), vp, i64, vp]),
    "sr_raster_scratch_bytes": (i64, [i32, i32, i32]),
}

_lib = None


def _build_module():
    return _native.load_module("sr_build", os.path.join(_HERE, "csrc", "build.py"))


def lib():
    """Load (once) and return the ctypes library, by the rules of _native.load (sr_source_hash() == hash of csrc/*.hip, headers,
    build flags)."""
    global _lib
    if _lib is None and _DEV_LIB:
        _lib = _native.bind(C.CDLL(_DEV_LIB), SYMBOLS)
    if _lib is None:
        _lib = _native.load(LIB_PATH, SYMBOLS, _build_module(), "sr_source_hash", "python stable-renderer_amd/csrc/build.py")
    return _lib


def check(rc):
    if rc != 0:
        _native.fail(rc, "libsr_hip", lib().sr_last_error())
