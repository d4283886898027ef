"""ctypes bindings of the nart_amd C ABI (include/nart_scene.h, include/nart_hip.h).

Mirrors the reference's host surface for the render path:
    Scene(path)                        <- Scene::Scene (src/core/scene.cpp:3-26)
    parse_args(argv) / load_sessions   <- ParseRenderParamArguments / LoadSessions (render.cpp:236-414)
    HipRenderer(scene).render(params)  <- RenderSession::Render (render.cpp:114-206), on the GPU
    write_exr(path, params, image)     <- RenderSession::WriteImageToEXR (render.cpp:208-234)
The render path has no CPU fallback: without the HIP library (or a GPU) it raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

NART_OK = 0
ERRORS = {-1: "NART_E_INVALID", -2: "NART_E_IO", -3: "NART_E_HIP", -4: "NART_E_OOM", -5: "NART_E_RCCL",
          -6: "NART_E_UNSUPPORTED"}
NART_E_UNSUPPORTED = -6

PIXEL_FLOATS = 5  # struct Pixel { vec4 contribution; float filterWeightSum; } (render.h:18-21)


class NativeLibraryMissing(RuntimeError):
    pass


class NartError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s (%d)%s" % (ERRORS.get(code, "error"), code, (": " + msg) if msg else ""))
        self.code = code


class RenderParams(ctypes.Structure):
    """struct RenderParams (include/nart/core/scene.h:25-36)."""
    _fields_ = [("integrator", ctypes.c_int32), ("image_width", ctypes.c_uint32), ("image_height", ctypes.c_uint32),
                ("bucket_size", ctypes.c_uint32), ("spp", ctypes.c_uint32), ("bounces", ctypes.c_uint32),
                ("filter_width", ctypes.c_float), ("roughening_factor", ctypes.c_float)]

    def __repr__(self):
        return "RenderParams(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_)

    def copy(self):
        p = RenderParams()
        ctypes.pointer(p)[0] = self
        return p


class SessionGeometry(ctypes.Structure):
    _fields_ = [("filter_bounds", ctypes.c_uint32), ("tile_size", ctypes.c_uint32), ("total_width", ctypes.c_uint32),
                ("total_height", ctypes.c_uint32), ("n_buckets_x", ctypes.c_uint32), ("n_buckets_y", ctypes.c_uint32)]


class BvhInfo(ctypes.Structure):
    """nart_bvh_info (include/nart_hip.h)."""
    _fields_ = [("num_nodes", ctypes.c_uint32), ("stack_depth", ctypes.c_uint32), ("num_leaf_tris", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class BvhDumpInfo(ctypes.Structure):
    """nart_bvh_dump_info (include/nart_hip.h)."""
    _fields_ = [("num_nodes", ctypes.c_uint32), ("num_leaf_tris", ctypes.c_uint32), ("stack_depth", ctypes.c_uint32),
                ("root_code", ctypes.c_int32), ("pad", ctypes.c_float), ("on_device", ctypes.c_uint32)]


# BVHNode (csrc/device/dscene.h), 64 B: two child boxes, two child codes (>= 0 an inner node, < 0 a
# leaf ~(first << 5 | (count - 1)))
BVH_NODE_DTYPE = np.dtype([("lo0", np.float32, 3), ("hi0", np.float32, 3), ("lo1", np.float32, 3),
                           ("hi1", np.float32, 3), ("child", np.int32, 2), ("pad", np.int32, 2)])


# nart_render_stats.schedule bits (include/nart_hip.h NART_SCHED_*)
SCHED = {"probe_queue": 0x1, "priority": 0x2, "spec_pairs": 0x4, "wave_groups": 0x8, "vol_queue": 0x10,
         "vol_sparse": 0x20, "splat_skew": 0x40, "primary": 0x80, "splat_rows": 0x100,
         "half_waves": 0x200, "specialized": 0x400,
         "lean": 0x800}

# scene feature bits (include/nart_hip.h NART_FT_*; nart_hip_scene_features)
FEATURES = {"lambert": 0x1, "specular": 0x2, "glass": 0x4, "glossy": 0x8, "plastic": 0x10, "disk": 0x20,
            "ring": 0x40, "environment": 0x80, "texture": 0x100, "normal_map": 0x200}
FT_ALL = 0x3FF
# device probe ops (include/nart_hip.h NART_EVAL_*; HipRenderer.eval, oracle.eval)
EVAL_OPS = {"acosf": 0, "atanf": 1, "atan2f": 2, "logf": 3, "logf_lds": 4, "sincos": 5, "f2u32": 6, "f2u8": 7,
            "gmod": 8, "gfract": 9, "rng_float": 10, "rng_int": 11, "uniform_sample_disk": 12,
            "uniform_sample_ring": 13, "cosine_sample_hemisphere": 14, "uniform_sample_sphere": 15,
            "sample_wh": 16, "fresnel": 17, "bxdf_f": 18, "bxdf_pdf": 19, "bxdf_f_pdf": 20, "bxdf_sample_f": 21}
EVAL_WORDS = 16  # floats per probe record (NART_EVAL_WORDS)
# nart_hip_trace (include/nart_hip.h): the traversal entry point that answers, and its records
TRACE_VARIANTS = {"plain": 0, "lds": 1, "step": 2, "step_rot": 3, "packet": 4}
TRACE_IN_WORDS, TRACE_OUT_WORDS, TRACE_NO_HIT = 8, 32, 0xFFFFFFFF
TRACE_CLOSEST, TRACE_ANY = 0, 1


def trace_rays(o, d, tmax=np.inf, kind=TRACE_CLOSEST):
    """(n, 8) float32 records of nart_hip_trace / oracle_trace_n from origins and directions (n, 3),
    tmax and query kind (scalars or (n,))."""
    o = np.asarray(o, np.float32).reshape(-1, 3)
    r = np.zeros((len(o), TRACE_IN_WORDS), np.float32)
    r[:, 0:3] = o
    r[:, 3] = np.asarray(tmax, np.float32)
    r[:, 4:7] = np.asarray(d, np.float32).reshape(-1, 3)
    r[:, 7] = np.broadcast_to(np.asarray(kind, np.uint32), (len(o),)).copy().view(np.float32)
    return r
# nart_hip_scene_eval (include/nart_hip.h NART_SCENE_*; HipRenderer.scene_eval, oracle.scene_eval): ops,
# record sizes and the (ENV, feature mask) builds of the path kernels its light and BSDF ops are compiled for
SCENE_OPS = {"tex_fetch": 0, "env_pdf": 1, "light_li": 2, "light_bound": 3, "light_sample_li": 4, "create_bsdf": 5,
             "dg_lookup": 6, "medium_walk": 7}
SCENE_IN_WORDS, SCENE_OUT_WORDS, SCENE_WALK_SEGMENTS = 16, 32, 7
SCENE_BUILDS = {"env_all": 0, "all": 1, "diffuse": 2, "glass": 3, "envtex": 4}
SCENE_BUILD_MASKS = {"env_all": (True, FT_ALL), "all": (False, FT_ALL), "diffuse": (False, 0x21),
                     "glass": (False, 0x25), "envtex": (True, 0x391)}


def scene_builds_fitting(features, has_env):
    """The SCENE_BUILDS a scene with this feature mask fits, by the renderer's rule (host/path_build.h
    plan_build): the mask covers the scene's, a narrow build goes with the scene's has_env, and a build
    without the environment code never meets an environment light."""
    out = []
    for name, (env, fm) in SCENE_BUILD_MASKS.items():
        if features & ~fm:
            continue
        if (env or not has_env) if fm == FT_ALL else (env == has_env):
            out.append(name)
    return out


# the feature masks the probe's templated ops are built for, with the BxDF kinds each creates
# (path.h create_bsdf: 0 Lambert, 1 specular, 2 specular dielectric, 3 dielectric, 4 Torrance-Sparrow)
EVAL_MASKS = {"all": (FT_ALL, (0, 1, 2, 3, 4)), "lambert": (0x1, (0,)), "specular": (0x2, (1, 4)),
              "glass": (0x4, (2, 3)), "glossy": (0x8, (1, 4)), "plastic": (0x10, (0, 1, 4))}
LIGHT_GROUPS_MAX = 8  # include/nart_hip.h NART_LIGHT_GROUPS_MAX
DEPTH_CUTS_MAX = 8  # include/nart_hip.h NART_DEPTH_CUTS_MAX


class RenderStats(ctypes.Structure):
    _fields_ = [("render_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double), ("splat_ms", ctypes.c_double),
                ("kernel_launches", ctypes.c_uint32), ("schedule", ctypes.c_uint32), ("samples", ctypes.c_uint64),
                ("traced_samples", ctypes.c_uint64), ("rays_extend", ctypes.c_uint64), ("rays_shadow", ctypes.c_uint64),
                ("node_visits", ctypes.c_uint64), ("tri_tests", ctypes.c_uint64), ("bounces", ctypes.c_uint64),
                ("latin_ms", ctypes.c_double), ("octree_checks", ctypes.c_uint64),
                ("octree_replays", ctypes.c_uint64), ("primary_ms", ctypes.c_double)]

    def schedule_names(self):
        return sorted(k for k, v in SCHED.items() if self.schedule & v)

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_P = ctypes.c_void_p


class _StageParams(ctypes.Structure):
    """What the five parameter structs of the whole-image stages share: Class.defaults() is the C ABI's
    init function named by the subclass (_init), keyword arguments override single fields."""
    _init = None

    @classmethod
    def defaults(cls, **kw):
        sp = cls()
        getattr(hip_lib(), cls._init)(ctypes.byref(sp))
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, ", ".join("%s=%r" % (f, getattr(self, f)) for f, _ in self._fields_))


class DenoiseParams(_StageParams):
    """nart_denoise_params (include/nart_hip.h); DenoiseParams.defaults() is
    nart_hip_denoise_params_init, keyword arguments override single fields."""
    _fields_ = [("iterations", ctypes.c_uint32), ("normal_squarings", ctypes.c_uint32),
                ("sigma_color", ctypes.c_float), ("sigma_depth", ctypes.c_float), ("depth_eps", ctypes.c_float),
                ("sigma_coverage", ctypes.c_float), ("albedo_floor", ctypes.c_float)]
    _init = "nart_hip_denoise_params_init"


class AdaptiveParams(_StageParams):
    """nart_adaptive_params (include/nart_hip.h, "Adaptive sampling"); AdaptiveParams.defaults() is
    nart_hip_adaptive_params_init, keyword arguments override single fields."""
    _fields_ = [("min_spp", ctypes.c_uint32), ("growth", ctypes.c_uint32), ("threshold", ctypes.c_float),
                ("floor", ctypes.c_float)]
    _init = "nart_hip_adaptive_params_init"


class CascadeParams(_StageParams):
    """nart_cascade_params (include/nart_hip.h, "Firefly cascade"); CascadeParams.defaults() is
    nart_hip_cascade_defaults, keyword arguments override single fields."""
    _fields_ = [("layers", ctypes.c_uint32), ("start", ctypes.c_float), ("base", ctypes.c_float),
                ("kappa", ctypes.c_float)]
    _init = "nart_hip_cascade_defaults"


class MatteParams(_StageParams):
    """nart_matte_params (include/nart_hip.h, "First-hit ID mattes"); MatteParams.defaults() is
    nart_hip_matte_defaults, keyword arguments override single fields."""
    _fields_ = [("kind", ctypes.c_uint32), ("ranks", ctypes.c_uint32)]
    _init = "nart_hip_matte_defaults"


MATTE_MESH, MATTE_MATERIAL = 0, 1  # NART_MATTE_* (include/nart_hip.h)


class GuideParams(_StageParams):
    """nart_guide_params (include/nart_hip.h, "Followed guides"); GuideParams.defaults() is
    nart_hip_guide_defaults, keyword arguments override single fields."""
    _fields_ = [("max_follow", ctypes.c_uint32)]
    _init = "nart_hip_guide_defaults"


class _Texture(ctypes.Structure):
    """nart_texture (include/nart_scene.h)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("rgba", _P)]


class Pattern(ctypes.Structure):
    """nart_pattern (include/nart_scene.h)."""
    _fields_ = [("type", ctypes.c_int32), ("value", ctypes.c_float * 3), ("texture", ctypes.c_int32),
                ("is_roughness", ctypes.c_int32)]


class Material(ctypes.Structure):
    """nart_material (include/nart_scene.h)."""
    _fields_ = [("type", ctypes.c_int32), ("has_normal", ctypes.c_int32), ("rho_d", Pattern), ("rho_s", Pattern),
                ("tau", Pattern), ("eta", Pattern), ("alpha", Pattern), ("normal", Pattern)]


MAT_LAMBERT, MAT_SPECULAR, MAT_GLASS, MAT_GLOSSY, MAT_PLASTIC = range(5)  # NART_MAT_*
PTN_CONSTANT, PTN_TEXTURE = 0, 1  # NART_PTN_*
AOV_ALBEDO, AOV_NORMAL = 0x1, 0x2  # NART_AOV_* (include/nart_hip.h)


class _BlobHead(ctypes.Structure):
    """Leading fields of nart_scene_blob (include/nart_scene.h)."""
    _fields_ = [("num_triangles", ctypes.c_uint32), ("num_meshes", ctypes.c_uint32),
                ("num_materials", ctypes.c_uint32), ("num_lights", ctypes.c_uint32),
                ("num_textures", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("triangles", _P),
                ("meshes", _P), ("materials", _P), ("lights", _P), ("textures", ctypes.POINTER(_Texture)),
                ("cam_fov", ctypes.c_float), ("cam_m", ctypes.c_float * 16)]


class Light(ctypes.Structure):
    """nart_light (include/nart_scene.h); m is the glm::mat4 storage of the light's transform."""
    _fields_ = [("type", ctypes.c_int32), ("radius", ctypes.c_float), ("inner_radius", ctypes.c_float),
                ("intensity", ctypes.c_float), ("Le", Pattern), ("m", ctypes.c_float * 16)]


LIGHT_DISK, LIGHT_RING, LIGHT_ENVIRONMENT = range(3)  # NART_LIGHT_*


class _Medium(ctypes.Structure):
    """nart_medium (include/nart_scene.h)."""
    _fields_ = [("present", ctypes.c_int32), ("bounds_min", ctypes.c_float * 3), ("bounds_max", ctypes.c_float * 3),
                ("sigma_a", ctypes.c_float), ("sigma_s", ctypes.c_float), ("Le", ctypes.c_float * 3),
                ("res", ctypes.c_uint32 * 3), ("density", _P)]


class _Blob(ctypes.Structure):
    """nart_scene_blob (include/nart_scene.h) whole: _BlobHead's fields, then the medium."""
    _fields_ = _BlobHead._fields_ + [("medium", _Medium)]


_SCENE_SIGS = {
    "nart_scene_load": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_P)]),
    "nart_scene_blob_of": (_P, [_P]),
    "nart_scene_free": (None, [_P]),
    "nart_scene_last_error": (ctypes.c_char_p, []),
    "nart_render_params_init": (None, [ctypes.POINTER(RenderParams)]),
    "nart_parse_args": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(RenderParams)]),
    "nart_load_sessions": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(RenderParams), ctypes.POINTER(RenderParams),
                                          ctypes.c_int]),
    "nart_session_geometry_of": (None, [ctypes.POINTER(RenderParams), ctypes.POINTER(SessionGeometry)]),
    "nart_filter_table": (None, [ctypes.POINTER(ctypes.c_float)]),
    "nart_combine_tiles": (None, [ctypes.POINTER(RenderParams), _P, _P]),
    "nart_write_exr": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(RenderParams), _P, ctypes.c_int]),
    "nart_float_to_half": (ctypes.c_uint16, [ctypes.c_float]),
    "nart_half_to_float": (ctypes.c_float, [ctypes.c_uint16]),
    "nart_read_exr_rgba": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(_P)]),
    "nart_free": (None, [_P]),
}
_HIP_SIGS = {
    "nart_hip_create": (ctypes.c_int, [_P, ctypes.c_int, ctypes.POINTER(_P)]),
    "nart_hip_destroy": (None, [_P]),
    "nart_hip_last_error": (ctypes.c_char_p, [_P]),
    "nart_hip_render": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, ctypes.POINTER(RenderStats)]),
    "nart_hip_render_aovs": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, _P, _P, _P,
                                            ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_moment": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, _P, _P, _P, _P,
                                              ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_halves": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, ctypes.POINTER(GuideParams),
                                              _P, _P, _P, _P, _P, ctypes.POINTER(RenderStats),
                                              ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_adaptive_params_init": (None, [ctypes.POINTER(AdaptiveParams)]),
    "nart_hip_adaptive_levels": (ctypes.c_int, [ctypes.POINTER(AdaptiveParams), ctypes.c_uint32,
                                                ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_render_adaptive": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(AdaptiveParams),
                                                ctypes.c_uint32, _P, _P, _P, _P, _P, _P, ctypes.POINTER(RenderStats),
                                                ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_cascade_defaults": (None, [ctypes.POINTER(CascadeParams)]),
    "nart_hip_cascade_levels": (ctypes.c_int, [ctypes.POINTER(CascadeParams), ctypes.POINTER(ctypes.c_float),
                                               ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_render_cascade": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(CascadeParams), _P, _P, _P,
                                               ctypes.POINTER(RenderStats)]),
    "nart_hip_cascade_reweight": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(CascadeParams), _P, _P,
                                                 _P]),
    "nart_hip_cascade_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_matte_defaults": (None, [ctypes.POINTER(MatteParams)]),
    "nart_hip_matte_ids": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_render_mattes": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(MatteParams), _P, _P, _P,
                                              ctypes.POINTER(RenderStats)]),
    "nart_hip_matte_rank": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(MatteParams), ctypes.c_uint32,
                                           _P, _P]),
    "nart_hip_matte_extract": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(MatteParams), _P,
                                              ctypes.c_uint64, _P]),
    "nart_hip_matte_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_light_groups": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, ctypes.c_uint32, ctypes.c_uint32,
                                                    _P, _P, ctypes.POINTER(RenderStats)]),
    "nart_hip_light_mix": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, _P, _P, _P]),
    "nart_hip_render_light_group_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, ctypes.c_uint32,
                                                           ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                           ctypes.c_uint32, ctypes.c_uint32, _P]),
    "nart_hip_light_group_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_depth_cuts": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, ctypes.c_uint32, _P, _P,
                                                  ctypes.POINTER(RenderStats)]),
    "nart_hip_depth_layers": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, _P, _P, _P]),
    "nart_hip_render_depth_cut_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, ctypes.c_uint32,
                                                         ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                         ctypes.c_uint32, _P]),
    "nart_hip_depth_cut_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_cost_grid": (ctypes.c_int, [ctypes.POINTER(RenderParams), ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_render_cost": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, _P, ctypes.POINTER(RenderStats)]),
    "nart_hip_render_cost_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, ctypes.c_uint32,
                                                    ctypes.c_uint32, ctypes.c_uint32, _P]),
    "nart_hip_cost_image": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, _P]),
    "nart_hip_cost_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_aov_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_uint32, ctypes.c_uint32, _P, _P]),
    "nart_hip_denoise_params_init": (None, [ctypes.POINTER(DenoiseParams)]),
    "nart_hip_denoise": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), _P, _P, _P, _P,
                                        ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_denoise_moment": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), _P, _P, _P,
                                               _P, _P, ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised_moment": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), _P,
                                                       _P, ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), _P, _P,
                                                ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_guide_defaults": (None, [ctypes.POINTER(GuideParams)]),
    "nart_hip_render_guides": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(GuideParams), ctypes.c_uint32,
                                              _P, _P, _P, _P, ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised_guides": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams),
                                                       ctypes.POINTER(GuideParams), ctypes.c_int, _P, _P,
                                                       ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_guide_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(GuideParams),
                                                     ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                     _P, _P, _P, _P]),
    "nart_hip_denoise_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_denoise_cross": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), _P, _P, _P, _P,
                                              _P, _P, _P, ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised_cross": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams),
                                                      ctypes.POINTER(GuideParams), _P, _P, _P, ctypes.POINTER(RenderStats),
                                                      ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_denoise_cross_timings": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                                      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_denoise_parts": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams), ctypes.c_uint32,
                                              _P, _P, _P, _P, _P, ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised_light_groups": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams),
                                                             ctypes.POINTER(GuideParams), _P, ctypes.c_uint32,
                                                             ctypes.c_uint32, _P, _P, _P, _P, ctypes.POINTER(RenderStats),
                                                             ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_render_denoised_depth_layers": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(DenoiseParams),
                                                             ctypes.POINTER(GuideParams), _P, ctypes.c_uint32, _P, _P, _P, _P,
                                                             ctypes.POINTER(RenderStats), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_denoise_parts_timings": (ctypes.c_int, [_P] + [ctypes.POINTER(ctypes.c_double)] * 6),
    "nart_hip_render_device": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(_P),
                                              ctypes.POINTER(RenderStats)]),
    "nart_hip_render_buckets_async": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.POINTER(ctypes.c_uint32),
                                                     ctypes.c_uint32, _P, _P, ctypes.POINTER(RenderStats)]),
    "nart_hip_combine_async": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), _P, _P, _P]),
    "nart_hip_render_samples": (ctypes.c_int, [_P, ctypes.POINTER(RenderParams), ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_uint32, _P]),
    "nart_hip_set_counters": (ctypes.c_int, [_P, ctypes.c_int]),
    "nart_hip_eval_sincos": (ctypes.c_int, [_P, _P, ctypes.c_uint32, _P, _P]),
    "nart_hip_eval": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_uint32, _P]),
    "nart_hip_trace": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, _P, ctypes.c_uint32, _P]),
    "nart_hip_scene_eval": (ctypes.c_int, [_P, ctypes.c_uint32, ctypes.c_uint32, _P, ctypes.c_uint32, _P]),
    "nart_hip_set_variant": (ctypes.c_int, [_P, ctypes.c_int]),
    "nart_hip_set_splat_mode": (ctypes.c_int, [_P, ctypes.c_int]),
    "nart_hip_set_specialize": (ctypes.c_int, [_P, ctypes.c_int]),
    "nart_hip_scene_features": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_scene_features_of": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_splat_thresholds": (ctypes.c_int, [ctypes.c_float, _P]),
    "nart_hip_env_search": (ctypes.c_int, [_P, ctypes.c_uint32, _P, ctypes.c_uint32, _P, _P]),
    "nart_hip_splat_lut": (ctypes.c_int, [ctypes.c_float, _P, ctypes.POINTER(ctypes.c_uint32),
                                          ctypes.POINTER(ctypes.c_uint32)]),
    "nart_hip_bvh_info": (ctypes.c_int, [_P, ctypes.POINTER(BvhInfo)]),
    "nart_hip_bvh_dump": (ctypes.c_int, [_P, ctypes.POINTER(BvhDumpInfo), _P, ctypes.c_size_t, _P, ctypes.c_size_t, _P,
                                         ctypes.c_size_t]),
    "nart_hip_context_bvh_dump": (ctypes.c_int, [_P, ctypes.POINTER(BvhDumpInfo), _P, ctypes.c_size_t, _P,
                                                 ctypes.c_size_t, _P, ctypes.c_size_t]),
    "nart_hip_create_multi": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_P)]),
    "nart_hip_context_devices": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "nart_hip_debug_fault": (ctypes.c_int, [_P, ctypes.c_int]),
    "nart_hip_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "nart_hip_context_bvh": (ctypes.c_int, [_P, ctypes.POINTER(BvhInfo), ctypes.POINTER(ctypes.c_double)]),
    "nart_hip_shard_buckets": (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
}
SCENE_SYMBOLS = tuple(_SCENE_SIGS)
HIP_SYMBOLS = tuple(_HIP_SIGS)

_libs = {}


def _load(name, sigs):
    if name in _libs:
        return _libs[name]
    path = os.path.join(LIB_DIR, name)
    if not os.path.exists(path):
        raise NativeLibraryMissing("%s not built (run nart_amd/build.py or __graft_entry__.build())" % path)
    lib = ctypes.CDLL(path)
    for fn, (res, args) in sigs.items():
        f = getattr(lib, fn)
        f.restype = res
        f.argtypes = args
    _libs[name] = lib
    return lib


def scene_lib():
    return _load("libnart_scene.so", _SCENE_SIGS)


def _missing_entry(fn, path):
    """Stand-in for an entry point an alternative build (NART_HIP_LIB) lacks: calling it raises
    a NartError naming the symbol and the build instead of an AttributeError or a call through an
    untyped pointer."""
    def call(*args):
        raise NartError(NART_E_UNSUPPORTED, "%s is not exported by the build %s" % (fn, path))
    return call


def hip_lib():
    # NART_HIP_LIB: an alternative build of the same ABI (A/B experiments, tools/ab.sh)
    alt = os.environ.get("NART_HIP_LIB")
    if alt:
        if "libnart_hip.so" not in _libs:
            scene_lib()  # its directory is on the alternative build's rpath too
            lib = ctypes.CDLL(os.path.abspath(alt))
            for fn, (res, args) in _HIP_SIGS.items():
                f = getattr(lib, fn, None)  # an older build may lack newer entry points
                if f is None:
                    setattr(lib, fn, _missing_entry(fn, alt))
                    continue
                f.restype = res
                f.argtypes = args
            _libs["libnart_hip.so"] = lib
        return _libs["libnart_hip.so"]
    return _load("libnart_hip.so", _HIP_SIGS)


def default_params():
    p = RenderParams()
    scene_lib().nart_render_params_init(ctypes.byref(p))
    return p


def parse_args(argv):
    """ParseRenderParamArguments: argv = [prog, scene, out, flags...]."""
    p = default_params()
    arr = (ctypes.c_char_p * len(argv))(*[a.encode() for a in argv])
    rc = scene_lib().nart_parse_args(len(argv), arr, ctypes.byref(p))
    if rc != NART_OK:
        raise NartError(rc, scene_lib().nart_scene_last_error().decode())
    return p


def load_sessions(path, cli=None):
    """LoadSessions: renderSessions[] resolved against CLI overrides."""
    lib = scene_lib()
    cli = cli if cli is not None else default_params()
    n = lib.nart_load_sessions(path.encode(), ctypes.byref(cli), None, 0)
    if n < 0:
        raise NartError(n, lib.nart_scene_last_error().decode())
    out = (RenderParams * max(n, 1))()
    lib.nart_load_sessions(path.encode(), ctypes.byref(cli), out, n)
    return [out[i].copy() for i in range(n)]


def session_geometry(p):
    g = SessionGeometry()
    scene_lib().nart_session_geometry_of(ctypes.byref(p), ctypes.byref(g))
    return g


def cost_grid(p):
    """(grid_h, grid_w) of the cost grid of p (nart_hip_cost_grid): the traced pixels, x and y below
    min(bucket_size * n_buckets, total size)."""
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    rc = hip_lib().nart_hip_cost_grid(ctypes.byref(p), ctypes.byref(w), ctypes.byref(h))
    if rc:
        raise NartError(rc, "cost_grid: invalid parameters")
    return h.value, w.value


def filter_table():
    t = (ctypes.c_float * 64)()
    scene_lib().nart_filter_table(t)
    return np.ctypeslib.as_array(t).copy()


def combine_tiles(p, tiles):
    g = session_geometry(p)
    tiles = np.ascontiguousarray(tiles, dtype=np.float32)
    img = np.zeros((g.total_height, g.total_width, PIXEL_FLOATS), np.float32)
    scene_lib().nart_combine_tiles(ctypes.byref(p), tiles.ctypes.data, img.ctypes.data)
    return img


def write_exr(path, p, image, compression=3):
    image = np.ascontiguousarray(image, dtype=np.float32)
    rc = scene_lib().nart_write_exr(path.encode(), ctypes.byref(p), image.ctypes.data, compression)
    if rc != NART_OK:
        raise NartError(rc, scene_lib().nart_scene_last_error().decode())


def read_exr(path):
    """RGBA halves as float32 array (H, W, 4)."""
    lib = scene_lib()
    w, h, ptr = ctypes.c_uint32(), ctypes.c_uint32(), _P()
    rc = lib.nart_read_exr_rgba(path.encode(), ctypes.byref(w), ctypes.byref(h), ctypes.byref(ptr))
    if rc != NART_OK:
        raise NartError(rc, lib.nart_scene_last_error().decode())
    n = w.value * h.value * 4
    halves = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint16)), shape=(n,)).copy()
    lib.nart_free(ptr)
    return halves.view(np.float16).astype(np.float32).reshape(h.value, w.value, 4)


def bvh_info(scene):
    """Host only: the BVH a render context would build for `scene` (nart_hip_bvh_info)."""
    info = BvhInfo()
    rc = hip_lib().nart_hip_bvh_info(_P(scene.blob), ctypes.byref(info))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_bvh_info")
    return {"num_nodes": info.num_nodes, "stack_depth": info.stack_depth, "num_leaf_tris": info.num_leaf_tris}


def _bvh_dump(entry, handle):
    """The two-call protocol of nart_hip_bvh_dump / nart_hip_context_bvh_dump: sizes, then the copy."""
    info = BvhDumpInfo()
    rc = entry(handle, ctypes.byref(info), None, 0, None, 0, None, 0)
    if rc != NART_OK:
        raise NartError(rc, "BVH dump (size query)")
    nn, nt = info.num_nodes, info.num_leaf_tris
    nodes = np.zeros(max(nn, 1), BVH_NODE_DTYPE)
    isect = np.zeros((max(nt, 1), 16), np.float32)
    perm = np.zeros((3, max(nt, 1), 16), np.float32)
    rc = entry(handle, ctypes.byref(info), nodes.ctypes.data, nn, isect.ctypes.data, nt * 16, perm.ctypes.data,
               nt * 48)
    if rc != NART_OK:
        raise NartError(rc, "BVH dump")
    return {"nodes": nodes[:nn], "tri_isect": isect[:nt], "tri_perm": perm[:, :nt], "root_code": int(info.root_code),
            "pad": np.float32(info.pad), "stack_depth": int(info.stack_depth), "num_nodes": int(nn),
            "num_leaf_tris": int(nt), "on_device": bool(info.on_device)}


def bvh_dump(scene):
    """Host only (test hook, nart_hip_bvh_dump): the binned-SAH tree a render context builds for `scene`
    by default, as a dict of numpy arrays: "nodes" (a structured array lo0, hi0, lo1, hi1, child, pad),
    "tri_isect" (num_leaf_tris, 16) float32 records in leaf order, "tri_perm" (3, num_leaf_tris, 16) the
    records permuted per ray major axis, and "root_code", "pad" (float32: what the child boxes were
    grown by), "stack_depth", "num_nodes", "num_leaf_tris", "on_device"."""
    return _bvh_dump(hip_lib().nart_hip_bvh_dump, _P(scene.blob))


class Scene:
    """Scene::Scene(path): JSON + .geo + EXR ingestion into the flat nart_scene_blob."""

    def __init__(self, path):
        self.path = path
        self._lib = scene_lib()
        self._h = _P()
        rc = self._lib.nart_scene_load(path.encode(), ctypes.byref(self._h))
        if rc != NART_OK:
            raise NartError(rc, self._lib.nart_scene_last_error().decode())
        self.blob = self._lib.nart_scene_blob_of(self._h)

    def counts(self):
        c = ctypes.cast(self.blob, ctypes.POINTER(ctypes.c_uint32))
        return {"triangles": c[0], "meshes": c[1], "materials": c[2], "lights": c[3], "textures": c[4]}

    def _view(self):
        return ctypes.cast(self.blob, ctypes.POINTER(_BlobHead)).contents

    def triangles(self):
        """(n, 24) float32 copy of the blob's triangles (nart_triangle: v0 v1 v2 n0 n1 n2 uv0 uv1 uv2)."""
        h = self._view()
        if not h.num_triangles:
            return np.zeros((0, 24), np.float32)
        return np.ctypeslib.as_array(ctypes.cast(h.triangles, ctypes.POINTER(ctypes.c_float)),
                                     shape=(h.num_triangles * 24,)).copy().reshape(-1, 24)

    def camera(self):
        """(fov, m): the camera's fov and glm::mat4 storage (16 float32; pinholecamera.cpp:3-40)."""
        h = self._view()
        return float(h.cam_fov), np.array(list(h.cam_m), np.float32)

    def materials(self):
        """Copies of the blob's nart_material records (Material: type, has_normal and the Pattern
        fields rho_d, rho_s, tau, eta, alpha, normal), in scene order."""
        h = self._view()
        src = ctypes.cast(h.materials, ctypes.POINTER(Material))
        out = []
        for i in range(h.num_materials):
            m = Material()
            ctypes.pointer(m)[0] = src[i]
            out.append(m)
        return out

    def meshes(self):
        """(n, 4) uint32 copy of the blob's nart_mesh records: first_tri, num_tris, material, priority."""
        h = self._view()
        if not h.num_meshes:
            return np.zeros((0, 4), np.uint32)
        return np.ctypeslib.as_array(ctypes.cast(h.meshes, ctypes.POINTER(ctypes.c_uint32)),
                                     shape=(h.num_meshes * 4,)).copy().reshape(-1, 4)

    def textures(self):
        """Loaded textures as (H, W, 4) uint16 half bit patterns (top row first), in load order."""
        h = self._view()
        out = []
        for i in range(h.num_textures):
            t = h.textures[i]
            out.append(np.ctypeslib.as_array(ctypes.cast(t.rgba, ctypes.POINTER(ctypes.c_uint16)),
                                             shape=(t.height * t.width * 4,)).copy().reshape(t.height, t.width, 4))
        return out

    def lights(self):
        """Copies of the blob's nart_light records (Light: type, radius, inner_radius, intensity, Le, m),
        in scene order."""
        h = self._view()
        src = ctypes.cast(h.lights, ctypes.POINTER(Light))
        out = []
        for i in range(h.num_lights):
            L = Light()
            ctypes.pointer(L)[0] = src[i]
            out.append(L)
        return out

    def medium(self):
        """The camera medium (nart_medium) as a dict -- bounds_min, bounds_max, sigma_a, sigma_s, Le, res
        (x, y, z) and density as a (rz, ry, rx) float32 copy -- or None without one."""
        m = ctypes.cast(self.blob, ctypes.POINTER(_Blob)).contents.medium
        if not m.present:
            return None
        rx, ry, rz = m.res
        dens = np.ctypeslib.as_array(ctypes.cast(m.density, ctypes.POINTER(ctypes.c_float)), shape=(rx * ry * rz,))
        return {"bounds_min": np.array(m.bounds_min[:], np.float32), "bounds_max": np.array(m.bounds_max[:], np.float32),
                "sigma_a": m.sigma_a, "sigma_s": m.sigma_s, "Le": np.array(m.Le[:], np.float32), "res": (rx, ry, rz),
                "density": dens.copy().reshape(rz, ry, rx)}

    def close(self):
        if self._h:
            self._lib.nart_scene_free(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene_features(scene):
    """Host only: the NART_FT_* feature mask a context would derive for the scene (it selects the
    scene-specialised path-kernel build; nart_hip_scene_features_of)."""
    m = ctypes.c_uint32()
    rc = hip_lib().nart_hip_scene_features_of(scene.blob, ctypes.byref(m))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_scene_features_of")
    return m.value


def shard_buckets(n_buckets_x, n_buckets, n_devices, device_index):
    """Host only: the bucket ids a multi-device context renders on device_index (diagonal lattice,
    nart_hip_shard_buckets; the same partition as nart_amd.dist.bucket_owners)."""
    lib = hip_lib()
    cnt = ctypes.c_uint32()
    rc = lib.nart_hip_shard_buckets(n_buckets_x, n_buckets, n_devices, device_index, None, ctypes.byref(cnt))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_shard_buckets")
    ids = np.zeros(max(1, cnt.value), np.uint32)
    lib.nart_hip_shard_buckets(n_buckets_x, n_buckets, n_devices, device_index,
                               ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(cnt))
    return ids[:cnt.value]


class HipRenderer:
    """nart_ctx: the scene resident on one GPU (device) or on several (devices=[...], one
    process, library-owned RCCL gather: nart_hip_create_multi); Render()-equivalent entry points."""

    def __init__(self, scene, device=0, variant=None, splat_mode=None, devices=None):
        self._lib = hip_lib()
        self.scene = scene
        self.device = device if devices is None else devices[0]
        self._ctx = _P()
        if devices is None:
            rc = self._lib.nart_hip_create(scene.blob, device, ctypes.byref(self._ctx))
        else:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = self._lib.nart_hip_create_multi(scene.blob, arr, len(devices), ctypes.byref(self._ctx))
        if rc != NART_OK:
            raise NartError(rc, "nart_hip_create failed on device(s) %s" % (devices if devices is not None else device))
        if variant is not None:
            self.set_variant(variant)
        if splat_mode is not None:
            self.set_splat_mode(splat_mode)

    def set_variant(self, variant):
        """0 = megakernel with a wave ray queue (default), 3 = megakernel with one lane per pixel;
        identical results (1, the wavefront variant, and 2, the traversal-quorum megakernel, were
        retired)."""
        self._check(self._lib.nart_hip_set_variant(self._ctx, int(variant)))

    def set_splat_mode(self, mode):
        """-1 = automatic (default: the skewed-time splat on launches of >= 1 wave per SIMD, else
        its W-lanes-per-column form), 5 = skewed time with W lanes per tile column, 4 = skewed-time
        splat, 3 = four tile pixels per lane, 1-0 = one pixel per lane (include/nart_hip.h);
        identical results."""
        self._check(self._lib.nart_hip_set_splat_mode(self._ctx, int(mode)))

    def set_specialize(self, mode):
        """Path-kernel builds: 0 (or False) the generic build, 1 the scene-specialised builds, 2 (or
        True, the default) those plus the lean three-waves-per-SIMD build of throughput-bound
        launches; identical results (nart_hip_set_specialize)."""
        self._check(self._lib.nart_hip_set_specialize(self._ctx, int(mode) if not isinstance(mode, bool)
                                                      else (2 if mode else 0)))

    def scene_features(self):
        """(the scene's feature mask, the mask of the path-kernel build the last render launched;
        FT_ALL = generic), NART_FT_* bits (nart_hip_scene_features)."""
        f, b = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.nart_hip_scene_features(self._ctx, ctypes.byref(f), ctypes.byref(b)))
        return f.value, b.value

    def _check(self, rc):
        if rc != NART_OK:
            raise NartError(rc, self._lib.nart_hip_last_error(self._ctx).decode())

    def bvh(self):
        """The acceleration structure this context built (nart_hip_context_bvh)."""
        info, ms = BvhInfo(), ctypes.c_double()
        self._check(self._lib.nart_hip_context_bvh(self._ctx, ctypes.byref(info), ctypes.byref(ms)))
        return {"num_nodes": info.num_nodes, "stack_depth": info.stack_depth, "num_leaf_tris": info.num_leaf_tris,
                "on_device": bool(info.reserved), "build_ms": ms.value}

    def bvh_dump(self):
        """Test hook (nart_hip_context_bvh_dump): the tree this context built (host SAH or device
        LBVH; a multi-device context's first device), copied to the host, as bvh_dump(scene) returns it."""
        return _bvh_dump(self._lib.nart_hip_context_bvh_dump, self._ctx)

    def devices(self):
        """(number of devices, gather over RCCL) of this context."""
        n, r = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.nart_hip_context_devices(self._ctx, ctypes.byref(n), ctypes.byref(r)))
        return n.value, r.value == 1

    def gather_mode(self):
        """"rccl", "copy", or "copy-fallback" (RCCL requested implicitly but unavailable)."""
        n, r = ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.nart_hip_context_devices(self._ctx, ctypes.byref(n), ctypes.byref(r)))
        return {1: "rccl", 0: "copy", 2: "copy-fallback"}[r.value]

    def debug_fault(self, fault):
        """Test hook (nart_hip_debug_fault): 1 = the next RCCL gather posts an invalid peer."""
        self._check(self._lib.nart_hip_debug_fault(self._ctx, int(fault)))

    def set_counters(self, on):
        self._check(self._lib.nart_hip_set_counters(self._ctx, 1 if on else 0))

    def render(self, p, stats=None):
        """Whole session -> (totalH, totalW, 5) float32 image of Pixels (host)."""
        g = session_geometry(p)
        img = np.empty((g.total_height, g.total_width, PIXEL_FLOATS), np.float32)
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render(self._ctx, ctypes.byref(p), img.ctypes.data, ctypes.byref(st)))
        return img

    def render_aovs(self, p, albedo=True, normal=True, beauty=True, stats=None, moment=False):
        """First-hit AOVs (nart_hip_render_aovs): a dict with (totalH, totalW, 5) float32 images under
        "albedo" ({albedo.rgb, coverage}), "normal" ({shading normal.xyz, depth}: a filtered average,
        not renormalised) and "beauty" (bit-identical to render()), each only if requested, plus
        "aov_ms", the device time of the AOV kernels.  finalize() of an image is the filtered AOV.
        beauty=False renders the AOVs alone (no path kernel).
        moment=True (nart_hip_render_moment) adds "moment", the second-moment image ({sum r^2 w,
        sum g^2 w, sum b^2 w, sum w^2} and the beauty's filter weight sum; sample_variance() turns it
        into a variance), and "moment_ms", the device time of its pass.  It needs the path kernel, so
        with beauty=False it is NART_E_INVALID; albedo and normal may both be False."""
        if moment and not beauty:
            raise NartError(-1, "the moment image needs the path kernel: beauty=False cannot be combined with moment=True")
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {}
        for name, want in (("beauty", beauty), ("albedo", albedo), ("normal", normal), ("moment", moment)):
            if want:
                out[name] = np.empty(shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        ms, mms = ctypes.c_double(), ctypes.c_double()
        mask = (AOV_ALBEDO if albedo else 0) | (AOV_NORMAL if normal else 0)
        if moment:
            self._check(self._lib.nart_hip_render_moment(self._ctx, ctypes.byref(p), mask, ptr("beauty"), ptr("albedo"),
                                                         ptr("normal"), ptr("moment"), ctypes.byref(st),
                                                         ctypes.byref(ms), ctypes.byref(mms)))
            out["moment_ms"] = mms.value
        else:
            self._check(self._lib.nart_hip_render_aovs(self._ctx, ctypes.byref(p), mask, ptr("beauty"), ptr("albedo"),
                                                       ptr("normal"), ctypes.byref(st), ctypes.byref(ms)))
        out["aov_ms"] = ms.value
        return out

    def render_adaptive(self, p, params=None, albedo=False, normal=False, moment=False, stats=None):
        """Adaptive sampling (nart_hip_render_adaptive; include/nart_hip.h has the algorithm): a pilot
        pass at params.min_spp, then only the buckets whose error exceeds params.threshold again at
        growth times the samples, up to p.spp.  params an AdaptiveParams (None: the defaults).
        Returns a dict with "beauty", the requested "albedo" / "normal" / "moment" images (as
        render_aovs() returns them; every bucket's share has the bits of a uniform render at the
        sample count the bucket ended on), "bucket_spp" (uint32) and "bucket_error" (float32, the
        error of the bucket's final level), both of shape (n_buckets_y, n_buckets_x), "levels" (the
        sample counts of the levels) and "adaptive_ms", the device time of the error and scatter
        kernels.  stats.samples is the number of samples taken over all levels."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {}
        for name, want in (("beauty", True), ("albedo", albedo), ("normal", normal), ("moment", moment)):
            if want:
                out[name] = np.empty(shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        out["bucket_spp"] = np.zeros((g.n_buckets_y, g.n_buckets_x), np.uint32)
        out["bucket_error"] = np.zeros((g.n_buckets_y, g.n_buckets_x), np.float32)
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        mask = (AOV_ALBEDO if albedo else 0) | (AOV_NORMAL if normal else 0)
        self._check(self._lib.nart_hip_render_adaptive(
            self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None, mask, ptr("beauty"), ptr("albedo"),
            ptr("normal"), ptr("moment"), out["bucket_spp"].ctypes.data, out["bucket_error"].ctypes.data,
            ctypes.byref(st), ctypes.byref(ms)))
        out["levels"] = adaptive_levels(params, p.spp)
        out["adaptive_ms"] = ms.value
        return out

    def _cascade_timings(self, out):
        c, w = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.nart_hip_cascade_timings(self._ctx, ctypes.byref(c), ctypes.byref(w)))
        out["cascade_ms"], out["reweight_ms"] = c.value, w.value
        return out

    def render_robust(self, p, params=None, with_beauty=False, with_layers=False, stats=None):
        """Firefly cascade (nart_hip_render_cascade; include/nart_hip.h has the definition): every
        sample is split by luminance between two neighbouring brightness layers, and a layer counts
        in a pixel only as far as the pixel's 3x3 neighbourhood holds enough samples of about that
        brightness.  params a CascadeParams (None: the defaults).  Returns a dict with "robust", the
        (totalH, totalW, 5) float32 image {rgb, alpha, 1} in the cropped window and zero in the border
        (finalize() and write_exr() take it as they take a render); "beauty" (bit-identical to
        render()) and "layers" ((K, totalH, totalW, 5): the layer images, each with the beauty's filter
        weight sum) if requested; "levels" (float32 b_0 .. b_{K-1}); "cascade_ms", the device time of
        the split and layer splats, and "reweight_ms", that of the reweighting."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        levels = cascade_levels(params)
        out = {"robust": np.empty(shape, np.float32), "levels": levels}
        if with_beauty:
            out["beauty"] = np.empty(shape, np.float32)
        if with_layers:
            out["layers"] = np.empty((len(levels),) + shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_cascade(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                      ptr("robust"), ptr("beauty"), ptr("layers"), ctypes.byref(st)))
        return self._cascade_timings(out)

    def cascade_reweight(self, p, beauty, layers, params=None):
        """The cascade's reweighting alone over host images (nart_hip_cascade_reweight): beauty a
        (totalH, totalW, 5) float32 image and layers the (K, totalH, totalW, 5) layer images as
        render_robust(with_beauty=True, with_layers=True) returns them, K = params.layers; p gives
        the geometry and spp.  Returns a dict with "robust" and "reweight_ms"."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        K = len(cascade_levels(params))
        b = np.ascontiguousarray(beauty, dtype=np.float32)
        l = np.ascontiguousarray(layers, dtype=np.float32)
        if b.shape != shape or l.shape != (K,) + shape:
            raise ValueError("cascade_reweight: images of shape %s and %s, expected %s and %s"
                             % (b.shape, l.shape, shape, (K,) + shape))
        out = {"robust": np.empty(shape, np.float32)}
        self._check(self._lib.nart_hip_cascade_reweight(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                        b.ctypes.data, l.ctypes.data, out["robust"].ctypes.data))
        return self._cascade_timings(out)

    def _matte_timings(self, out):
        m, r = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.nart_hip_matte_timings(self._ctx, ctypes.byref(m), ctypes.byref(r)))
        out["matte_ms"], out["rank_ms"] = m.value, r.value
        return out

    def render_mattes(self, p, params=None, with_beauty=False, with_planes=False, stats=None):
        """First-hit ID mattes (nart_hip_render_mattes; include/nart_hip.h has the definition): per
        pixel the R = params.ranks greatest (id, coverage) pairs of the meshes or materials its camera
        samples hit first.  params a MatteParams (None: the defaults).  Returns a dict with "ranks", an
        (R/2, totalH, totalW, 5) float32 array (image k: {id_2k, c_2k, id_2k+1, c_2k+1, 1} in the
        cropped window, an empty rank is {-1, 0}; zero in the border; write_exr() takes each image as
        it takes a render); "n_ids"; "beauty" (bit-identical to render()) and "planes" ((P, totalH,
        totalW, 5): the coverage planes, four ids each, with the beauty's filter weight sum) if
        requested; "matte_ms", the device time of the plane passes, and "rank_ms", that of the ranking.
        Without with_beauty no path kernel is launched."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        mp = params if params is not None else MatteParams.defaults()
        n = ctypes.c_uint32()
        self._lib.nart_hip_matte_ids(self.scene.blob, mp.kind, ctypes.byref(n))  # the call below reports errors
        out = {"ranks": np.empty((max(1, mp.ranks // 2),) + shape, np.float32), "n_ids": n.value}
        if with_beauty:
            out["beauty"] = np.empty(shape, np.float32)
        if with_planes:
            out["planes"] = np.empty(((n.value + 3) // 4,) + shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_mattes(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                     ptr("ranks"), ptr("beauty"), ptr("planes"), ctypes.byref(st)))
        out["ranks"] = out["ranks"][:mp.ranks // 2]
        return self._matte_timings(out)

    def matte_rank(self, p, planes, n_ids, params=None):
        """The ranking alone over host planes (nart_hip_matte_rank): planes the (ceil(n_ids / 4), totalH,
        totalW, 5) float32 coverage planes as render_mattes(with_planes=True) returns them; p gives the
        geometry.  Returns a dict with "ranks" and "rank_ms"."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        mp = params if params is not None else MatteParams.defaults()
        P = (int(n_ids) + 3) // 4
        pl = np.ascontiguousarray(planes, dtype=np.float32).reshape((-1,) + shape)
        if pl.shape[0] != P:
            raise ValueError("matte_rank: %d planes, expected %d for %d ids" % (pl.shape[0], P, n_ids))
        out = {"ranks": np.empty((max(1, mp.ranks // 2),) + shape, np.float32)}
        self._check(self._lib.nart_hip_matte_rank(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                  int(n_ids), pl.ctypes.data if P else None, out["ranks"].ctypes.data))
        out["ranks"] = out["ranks"][:mp.ranks // 2]
        return self._matte_timings(out)

    def matte_extract(self, p, ranks, ids, params=None):
        """The coverage of an id set (nart_hip_matte_extract): ranks the (R/2, totalH, totalW, 5) rank
        images of render_mattes() or matte_rank() with the same params; ids an iterable of ids or an
        integer bit mask (bit m: id m).  Returns the (totalH, totalW, 5) float32 matte {m, m, m, m, 1}
        (zero in the border)."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        mp = params if params is not None else MatteParams.defaults()
        rk = np.ascontiguousarray(ranks, dtype=np.float32)
        if rk.shape != (mp.ranks // 2,) + shape:
            raise ValueError("matte_extract: rank images of shape %s, expected %s" % (rk.shape, (mp.ranks // 2,) + shape))
        mask = ids if isinstance(ids, int) else sum(1 << int(i) for i in set(ids))
        out = np.empty(shape, np.float32)
        self._check(self._lib.nart_hip_matte_extract(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                     rk.ctypes.data, mask & (2 ** 64 - 1), out.ctypes.data))
        return out

    def _light_group_timings(self, out):
        s, m = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.nart_hip_light_group_timings(self._ctx, ctypes.byref(s), ctypes.byref(m)))
        out["splat_ms"], out["mix_ms"] = s.value, m.value
        return out

    @staticmethod
    def _light_group_map(groups):
        """The group map as the ABI takes it: a uint32 array (None: null) and G = the largest group + 1."""
        if groups is None:
            return None, 0, 0
        m = np.ascontiguousarray(groups, dtype=np.uint32).reshape(-1)
        return m, len(m), int(m.max()) + 1 if len(m) else 0

    def render_light_groups(self, p, groups, with_beauty=False, stats=None, n_groups=None):
        """The beauty split by light from one render (nart_hip_render_light_groups; include/nart_hip.h
        has the definition): groups[l] is the group of the scene's light l, G = max(groups) + 1 unless
        n_groups says otherwise (at most 8).  Returns a dict with "groups", a (G, totalH, totalW, 5)
        float32 array -- image g holds the radiance of the lights of group g, bit-identical to a render
        with every other light's intensity at 0, alpha and filter weight sum the beauty's; "beauty"
        (bit-identical to render()) if requested; "splat_ms", the device time of the group splats."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        m, n, G = self._light_group_map(groups)
        G = G if n_groups is None else int(n_groups)
        out = {"groups": np.empty((max(1, G),) + shape, np.float32)}
        if with_beauty:
            out["beauty"] = np.empty(shape, np.float32)
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_light_groups(self._ctx, ctypes.byref(p), m.ctypes.data if m is not None else None,
                                                           n, G, out["groups"].ctypes.data,
                                                           out["beauty"].ctypes.data if with_beauty else None,
                                                           ctypes.byref(st)))
        out["groups"] = out["groups"][:G]
        return self._light_group_timings(out)

    def render_light_group_samples(self, p, groups, x0, y0, w, h, n_groups=None):
        """Per-sample group records of a rect in total-image coordinates
        (nart_hip_render_light_group_samples): (G, h, w, spp, 4) float32 = {Lg.rgb, alpha}."""
        m, n, G = self._light_group_map(groups)
        G = G if n_groups is None else int(n_groups)
        out = np.empty((max(1, G), h, w, p.spp, 4), np.float32)
        self._check(self._lib.nart_hip_render_light_group_samples(self._ctx, ctypes.byref(p),
                                                                  m.ctypes.data if m is not None else None, n, G, x0, y0,
                                                                  w, h, out.ctypes.data))
        return out[:G]

    def light_mix(self, p, images, gains):
        """The mix of group images (nart_hip_light_mix): images a (G, totalH, totalW, 5) float32 array as
        render_light_groups() returns it, gains one number per group or a (G, 3) array of r, g, b gains
        (finite).  Returns the (totalH, totalW, 5) float32 image: per channel the sum over g ascending
        of gains[g][c] * images[g][..., c] in float32, alpha and filter weight sum those of image 0."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        im = np.ascontiguousarray(images, dtype=np.float32)
        if im.ndim != 4 or im.shape[1:] != shape:
            raise ValueError("light_mix: images of shape %s, expected (G,) + %s" % (im.shape, shape))
        G = im.shape[0]
        k = np.asarray(gains, dtype=np.float32)
        k = np.ascontiguousarray(np.repeat(k[:, None], 3, axis=1) if k.ndim == 1 else k)
        if k.shape != (G, 3):
            raise ValueError("light_mix: gains of shape %s, expected (%d,) or (%d, 3)" % (k.shape, G, G))
        out = np.empty(shape, np.float32)
        self._check(self._lib.nart_hip_light_mix(self._ctx, ctypes.byref(p), G, k.ctypes.data, im.ctypes.data, out.ctypes.data))
        return out

    def light_group_timings(self):
        """Device times of the last light-group call: {"splat_ms", "mix_ms"}."""
        return self._light_group_timings({})

    def _depth_cut_timings(self, out):
        s, m = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.nart_hip_depth_cut_timings(self._ctx, ctypes.byref(s), ctypes.byref(m)))
        out["splat_ms"], out["layers_ms"] = s.value, m.value
        return out

    @staticmethod
    def _depth_cut_list(cuts):
        """The cuts as the ABI takes them: a uint32 array (None: null) and its length K."""
        if cuts is None:
            return None, 0
        c = np.ascontiguousarray(cuts, dtype=np.uint32).reshape(-1)
        return c, len(c)

    def render_depth_cuts(self, p, cuts, with_beauty=False, stats=None, n_cuts=None):
        """The image at lower bounce limits from one render (nart_hip_render_depth_cuts; include/nart_hip.h
        has the definition): cuts is a strictly ascending list of at most 8 bounce limits in 1..p.bounces
        (n_cuts overrides its length as the ABI sees it).  Returns a dict with "cuts", a
        (K, totalH, totalW, 5) float32 array -- image j holds every sample's radiance as it stood when
        the path had made cuts[j] bounces, alpha and filter weight sum the beauty's; a cut equal to
        p.bounces is the beauty; "beauty" (bit-identical to render()) if requested; "splat_ms", the
        device time of the cut splats."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        c, K = self._depth_cut_list(cuts)
        K = K if n_cuts is None else int(n_cuts)
        out = {"cuts": np.empty((max(1, K),) + shape, np.float32)}
        if with_beauty:
            out["beauty"] = np.empty(shape, np.float32)
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_depth_cuts(self._ctx, ctypes.byref(p), c.ctypes.data if c is not None else None,
                                                         K, out["cuts"].ctypes.data,
                                                         out["beauty"].ctypes.data if with_beauty else None,
                                                         ctypes.byref(st)))
        out["cuts"] = out["cuts"][:K]
        out["splat_ms"] = self._depth_cut_timings({})["splat_ms"]
        return out

    def render_depth_cut_samples(self, p, cuts, x0, y0, w, h, n_cuts=None):
        """Per-sample cut records of a rect in total-image coordinates
        (nart_hip_render_depth_cut_samples): (K, h, w, spp, 4) float32 = {L_d.rgb, alpha}."""
        c, K = self._depth_cut_list(cuts)
        K = K if n_cuts is None else int(n_cuts)
        out = np.empty((max(1, K), h, w, p.spp, 4), np.float32)
        self._check(self._lib.nart_hip_render_depth_cut_samples(self._ctx, ctypes.byref(p),
                                                                c.ctypes.data if c is not None else None, K, x0, y0, w, h,
                                                                out.ctypes.data))
        return out[:K]

    def depth_layers(self, p, cut_images, beauty):
        """The layers between cut images (nart_hip_depth_layers): cut_images a (K, totalH, totalW, 5)
        float32 array as render_depth_cuts() returns it, beauty the same call's beauty.  Returns the
        (K + 1, totalH, totalW, 5) float32 layers: the first cut, the float32 differences of neighbouring
        cuts, the beauty minus the last cut; alpha and filter weight sum those of the beauty."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        im = np.ascontiguousarray(cut_images, dtype=np.float32)
        b = np.ascontiguousarray(beauty, dtype=np.float32)
        if im.ndim != 4 or im.shape[1:] != shape or b.shape != shape:
            raise ValueError("depth_layers: images of shape %s and %s, expected (K,) + %s and %s" % (im.shape, b.shape, shape, shape))
        K = im.shape[0]
        out = np.empty((K + 1,) + shape, np.float32)
        self._check(self._lib.nart_hip_depth_layers(self._ctx, ctypes.byref(p), K, im.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def depth_cut_timings(self):
        """Device times of the last depth-cut call: {"splat_ms", "layers_ms"}."""
        return self._depth_cut_timings({})

    def cost_timings(self):
        """Device times of the last cost call: {"reduce_ms", "image_ms"}."""
        r, m = ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.nart_hip_cost_timings(self._ctx, ctypes.byref(r), ctypes.byref(m)))
        return {"reduce_ms": r.value, "image_ms": m.value}

    def render_cost(self, p, with_beauty=False, stats=None, cost=True):
        """Per-pixel ray, hit and traversal counts of a render (nart_hip_render_cost; include/nart_hip.h,
        "Cost image", has the definition).  Returns a dict with "cost", the (grid_h, grid_w, 4) uint32
        grid of {extension rays, shadow rays, shaded hits, traversal steps} summed over each traced
        pixel's samples (cost_grid(p) gives its shape); "beauty" (bit-identical to render()) if requested;
        "totals", the four sums over the grid as Python ints; "buckets", the (n_buckets_y, n_buckets_x, 4)
        uint64 sums over each bucket's pixels; "reduce_ms", the device time of the reduces.  cost=False
        passes a null grid (the ABI's error)."""
        g = session_geometry(p)
        gh, gw = cost_grid(p)
        out = {"cost": np.zeros((gh, gw, 4), np.uint32)}
        if with_beauty:
            out["beauty"] = np.empty((g.total_height, g.total_width, PIXEL_FLOATS), np.float32)
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_cost(self._ctx, ctypes.byref(p), out["cost"].ctypes.data if cost else None,
                                                   out["beauty"].ctypes.data if with_beauty else None, ctypes.byref(st)))
        c = out["cost"]
        out["totals"] = tuple(int(v) for v in c.reshape(-1, 4).sum(axis=0, dtype=np.uint64))
        B = p.bucket_size
        edges_y, edges_x = np.arange(0, gh, B), np.arange(0, gw, B)
        rows = np.add.reduceat(c.astype(np.uint64), edges_y, axis=0)
        out["buckets"] = np.add.reduceat(rows, edges_x, axis=1)
        out["reduce_ms"] = self.cost_timings()["reduce_ms"]
        return out

    def render_cost_samples(self, p, x0, y0, w, h):
        """Per-sample cost records of a rect in total-image coordinates, which are the cost grid's
        (nart_hip_render_cost_samples): (h, w, spp, 4) uint32."""
        out = np.zeros((h, w, p.spp, 4), np.uint32)
        self._check(self._lib.nart_hip_render_cost_samples(self._ctx, ctypes.byref(p), x0, y0, w, h, out.ctypes.data))
        return out

    def cost_image(self, p, cost):
        """A cost grid as a (totalH, totalW, 5) float32 image (nart_hip_cost_image): grid pixel (x, y) at
        (y + fb, x + fb) as {the four counts as float32, spp}, zero elsewhere, so that finalize() gives the
        per-sample means over the cropped window and write_exr() takes it unchanged."""
        g = session_geometry(p)
        c = np.ascontiguousarray(cost, dtype=np.uint32)
        if c.shape != cost_grid(p) + (4,):
            raise ValueError("cost_image: grid of shape %s, expected %s" % (c.shape, cost_grid(p) + (4,)))
        out = np.empty((g.total_height, g.total_width, PIXEL_FLOATS), np.float32)
        self._check(self._lib.nart_hip_cost_image(self._ctx, ctypes.byref(p), c.ctypes.data, out.ctypes.data))
        return out

    def render_aov_samples(self, p, x0, y0, w, h):
        """Per-sample AOV records of a rect in total-image coordinates (nart_hip_render_aov_samples):
        (h, w, spp, 8) float32 = {albedo.rgb, hit, normal.xyz, depth} and (h, w, spp) uint32 first-hit
        triangle indices (0xFFFFFFFF: miss)."""
        out = np.empty((h, w, p.spp, 8), np.float32)
        tri = np.empty((h, w, p.spp), np.uint32)
        self._check(self._lib.nart_hip_render_aov_samples(self._ctx, ctypes.byref(p), x0, y0, w, h, out.ctypes.data,
                                                          tri.ctypes.data))
        return out, tri

    def render_guides(self, p, params=None, albedo=True, normal=True, beauty=True, moment=False, stats=None):
        """Followed guides (nart_hip_render_guides; include/nart_hip.h has the chain): as render_aovs(),
        with "albedo" and "normal" taken at the first surface behind perfect mirrors and smooth
        dielectrics.  params a GuideParams (None: the defaults).  "guide_ms" is the device time of the
        guide kernel and the guide splats; "beauty" and "moment" have the bits render() and
        render_aovs(moment=True) give."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {}
        for name, want in (("beauty", beauty), ("albedo", albedo), ("normal", normal), ("moment", moment)):
            if want:
                out[name] = np.empty(shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        mask = (AOV_ALBEDO if albedo else 0) | (AOV_NORMAL if normal else 0)
        self._check(self._lib.nart_hip_render_guides(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                     mask, ptr("beauty"), ptr("albedo"), ptr("normal"), ptr("moment"),
                                                     ctypes.byref(st), ctypes.byref(ms)))
        out["guide_ms"] = ms.value
        return out

    def render_halves(self, p, albedo=False, normal=False, guides=None, stats=None):
        """Half buffers (nart_hip_render_halves; include/nart_hip.h has the definition): the beauty and
        the images of its samples of even and of odd index, from one render.  Returns a dict with
        "beauty" (bit-identical to render()), "halves" ((2, totalH, totalW, 5) float32: half h holds
        {sum w r, sum w g, sum w b, sum w} over its own samples and the beauty's filter weight sum;
        half_mean() gives its mean), the requested "albedo" / "normal" images -- the first-hit AOVs of
        render_aovs(), or with guides a GuideParams the followed guides of render_guides() -- and
        "halves_ms", the device time of the splits and the half splats."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {"beauty": np.empty(shape, np.float32), "halves": np.empty((2,) + shape, np.float32)}
        for name, want in (("albedo", albedo), ("normal", normal)):
            if want:
                out[name] = np.empty(shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        mask = (AOV_ALBEDO if albedo else 0) | (AOV_NORMAL if normal else 0)
        self._check(self._lib.nart_hip_render_halves(self._ctx, ctypes.byref(p), mask,
                                                     ctypes.byref(guides) if guides is not None else None, ptr("beauty"),
                                                     ptr("albedo"), ptr("normal"), out["halves"][0].ctypes.data,
                                                     out["halves"][1].ctypes.data, ctypes.byref(st), ctypes.byref(ms)))
        out["halves_ms"] = ms.value
        return out

    def render_guide_samples(self, p, x0, y0, w, h, params=None):
        """Per-sample guide chains of a rect in total-image coordinates (nart_hip_render_guide_samples),
        M = max_follow + 1: a dict with "rec" (h, w, spp, 8) float32 = {albedo record, normal record},
        "n_seg" (h, w, spp) uint32 segments traced (0: a camera-ray miss), "seg" (h, w, spp, M, 8)
        float32 = {o.xyz, tmax, d.xyz, t} and "tri" (h, w, spp, M) uint32 (0xFFFFFFFF: that segment
        missed or was never traced)."""
        gp = params if params is not None else GuideParams.defaults()
        M = int(gp.max_follow) + 1 if gp.max_follow <= 10 else 1  # (a bad value is the entry point's to refuse)
        out = {"rec": np.empty((h, w, p.spp, 8), np.float32), "n_seg": np.empty((h, w, p.spp), np.uint32),
               "seg": np.empty((h, w, p.spp, M, 8), np.float32), "tri": np.empty((h, w, p.spp, M), np.uint32)}
        self._check(self._lib.nart_hip_render_guide_samples(self._ctx, ctypes.byref(p), ctypes.byref(gp), x0, y0, w, h,
                                                            out["rec"].ctypes.data, out["seg"].ctypes.data,
                                                            out["tri"].ctypes.data, out["n_seg"].ctypes.data))
        return out

    def denoise(self, p, beauty, albedo, normal, params=None, moment=None):
        """Denoise host images (nart_hip_denoise): beauty, albedo and normal are (totalH, totalW, 5)
        float32 images as render_aovs() returns them; params a DenoiseParams (None: the defaults).
        Returns the denoised (totalH, totalW, 5) image: {rgb, alpha, 1} in the cropped window, zero
        in the border, so finalize() and write_exr() take it as they take a render.
        moment: the second-moment image of render_aovs(moment=True); the filter then takes each
        pixel's variance from it (nart_hip_denoise_moment; p.spp >= 2) instead of the spatial estimate."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        src = [np.ascontiguousarray(a, dtype=np.float32)
               for a in (beauty, albedo, normal) + (() if moment is None else (moment,))]
        for a in src:
            if a.shape != shape:
                raise ValueError("denoise: image of shape %s, expected %s" % (a.shape, shape))
        out = np.empty(shape, np.float32)
        dp = ctypes.byref(params) if params else None
        if moment is None:
            self._check(self._lib.nart_hip_denoise(self._ctx, ctypes.byref(p), dp, src[0].ctypes.data,
                                                   src[1].ctypes.data, src[2].ctypes.data, out.ctypes.data, None))
        else:
            self._check(self._lib.nart_hip_denoise_moment(self._ctx, ctypes.byref(p), dp, src[0].ctypes.data,
                                                          src[1].ctypes.data, src[2].ctypes.data, src[3].ctypes.data,
                                                          out.ctypes.data, None))
        return out

    def render_denoised(self, p, params=None, beauty=True, stats=None, sample_variance=False, guides=None):
        """Render the beauty and both first-hit AOVs and denoise them on the device
        (nart_hip_render_denoised): a dict with "denoised", "beauty" (the noisy image, bit-identical to
        render(); only if requested) and "denoise_ms", the device time of the denoise kernels.
        sample_variance=True also renders the second-moment image and denoises with the variance
        taken from it (nart_hip_render_denoised_moment; p.spp >= 2).
        guides: a GuideParams feeds the filter with the followed guides instead of the first-hit AOVs
        (nart_hip_render_denoised_guides); None is the first-hit call."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {"denoised": np.empty(shape, np.float32)}
        if beauty:
            out["beauty"] = np.empty(shape, np.float32)
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        dp = ctypes.byref(params) if params else None
        img = out["beauty"].ctypes.data if beauty else None
        if guides is not None:
            self._check(self._lib.nart_hip_render_denoised_guides(self._ctx, ctypes.byref(p), dp, ctypes.byref(guides),
                                                                  1 if sample_variance else 0, img,
                                                                  out["denoised"].ctypes.data, ctypes.byref(st),
                                                                  ctypes.byref(ms)))
        else:
            entry = self._lib.nart_hip_render_denoised_moment if sample_variance else self._lib.nart_hip_render_denoised
            self._check(entry(self._ctx, ctypes.byref(p), dp, img, out["denoised"].ctypes.data, ctypes.byref(st),
                              ctypes.byref(ms)))
        out["denoise_ms"] = ms.value
        return out

    def denoise_timings(self):
        """Device times (ms) of the last denoise, kernel by kernel (nart_hip_denoise_timings):
        {"prepare", "variance", "passes": [8], "finalize"}."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        passes = (ctypes.c_double * 8)()
        self._check(self._lib.nart_hip_denoise_timings(self._ctx, ctypes.byref(a), ctypes.byref(b), passes,
                                                       ctypes.byref(c)))
        return {"prepare": a.value, "variance": b.value, "passes": list(passes), "finalize": c.value}

    def denoise_cross(self, p, half_a, half_b, beauty, albedo, normal, params=None, with_error=True):
        """Cross-filtered denoising of host images (nart_hip_denoise_cross; include/nart_hip.h,
        "Cross-filtered denoising"): half_a, half_b and beauty as render_halves() returns them, albedo
        and normal as render_aovs() or render_guides() do; params a DenoiseParams (None: the defaults).
        Each half is filtered with colour weights taken from the other.  Returns a dict with "denoised",
        the average of the two filtered halves ({rgb, alpha, 1} in the cropped window, zero in the
        border), "error" unless with_error=False ({e.rgb, alpha, 1}: per channel the squared half
        difference of the filtered halves, a one-sample estimate of the squared error of "denoised")
        and "denoise_ms".  p.spp >= 2."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        src = [np.ascontiguousarray(a, dtype=np.float32) for a in (half_a, half_b, beauty, albedo, normal)]
        for a in src:
            if a.shape != shape:
                raise ValueError("denoise_cross: image of shape %s, expected %s" % (a.shape, shape))
        out = {"denoised": np.empty(shape, np.float32)}
        if with_error:
            out["error"] = np.empty(shape, np.float32)
        ms = ctypes.c_double()
        self._check(self._lib.nart_hip_denoise_cross(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                                                     *[a.ctypes.data for a in src], out["denoised"].ctypes.data,
                                                     out["error"].ctypes.data if with_error else None, ctypes.byref(ms)))
        out["denoise_ms"] = ms.value
        return out

    def render_denoised_cross(self, p, params=None, beauty=True, stats=None, guides=None):
        """Render the beauty, its two half buffers and both first-hit AOVs (guides a GuideParams: the
        followed guides) and cross-denoise them on the device (nart_hip_render_denoised_cross): a dict
        with "denoised", "error", "beauty" (bit-identical to render(); only if requested) and
        "denoise_ms".  The images are denoise_cross()'s over render_halves()' images.  p.spp >= 2."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {"denoised": np.empty(shape, np.float32), "error": np.empty(shape, np.float32)}
        if beauty:
            out["beauty"] = np.empty(shape, np.float32)
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        self._check(self._lib.nart_hip_render_denoised_cross(
            self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
            ctypes.byref(guides) if guides is not None else None, out["denoised"].ctypes.data, out["error"].ctypes.data,
            out["beauty"].ctypes.data if beauty else None, ctypes.byref(st), ctypes.byref(ms)))
        out["denoise_ms"] = ms.value
        return out

    def denoise_cross_timings(self):
        """Device times (ms) of the last cross denoise, kernel by kernel (nart_hip_denoise_cross_timings):
        {"prepare", "variance", "passes": [8], "finalize"}."""
        a, b, c = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        passes = (ctypes.c_double * 8)()
        self._check(self._lib.nart_hip_denoise_cross_timings(self._ctx, ctypes.byref(a), ctypes.byref(b), passes,
                                                             ctypes.byref(c)))
        return {"prepare": a.value, "variance": b.value, "passes": list(passes), "finalize": c.value}

    def denoise_parts(self, p, parts, albedo, normal, params=None, with_sum=False):
        """Denoise K host part images that share their guides (nart_hip_denoise_parts; include/nart_hip.h,
        "Denoised parts"): parts a (K, totalH, totalW, 5) float32 array, 1 <= K <= 9 -- light groups as
        render_light_groups() returns them, or layers as depth_layers() does -- albedo and normal as
        render_aovs() returns them; params a DenoiseParams (None: the defaults).  Returns the
        (K, totalH, totalW, 5) denoised parts, image k with the bits of denoise(p, parts[k], albedo, normal,
        params); with_sum=True returns (denoised, sum), the sum being ((d_0 + d_1) + d_2) + ... per r, g, b
        with the alpha and filter weight sum of d_0."""
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        im = np.ascontiguousarray(parts, dtype=np.float32)
        a, n = (np.ascontiguousarray(x, dtype=np.float32) for x in (albedo, normal))
        if im.ndim != 4 or im.shape[1:] != shape or a.shape != shape or n.shape != shape:
            raise ValueError("denoise_parts: images of shape %s, %s and %s, expected (K,) + %s and %s twice" % (
                im.shape, a.shape, n.shape, shape, shape))
        K = im.shape[0]
        out = np.empty((max(1, K),) + shape, np.float32)
        total = np.empty(shape, np.float32) if with_sum else None
        self._check(self._lib.nart_hip_denoise_parts(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None, K,
                                                     im.ctypes.data, a.ctypes.data, n.ctypes.data, out.ctypes.data,
                                                     total.ctypes.data if with_sum else None, None))
        return (out[:K], total) if with_sum else out[:K]

    def _denoised_parts_call(self, p, entry, head, K, noisy_name, params, guides, with_sum, with_noisy, with_beauty, stats):
        g = session_geometry(p)
        shape = (g.total_height, g.total_width, PIXEL_FLOATS)
        out = {"denoised": np.empty((max(1, K),) + shape, np.float32)}
        if with_sum:
            out["sum"] = np.empty(shape, np.float32)
        if with_noisy:
            out[noisy_name] = np.empty((max(1, K),) + shape, np.float32)
        if with_beauty:
            out["beauty"] = np.empty(shape, np.float32)
        ptr = lambda name: out[name].ctypes.data if name in out else None
        st = stats if stats is not None else RenderStats()
        ms = ctypes.c_double()
        self._check(entry(self._ctx, ctypes.byref(p), ctypes.byref(params) if params else None,
                          ctypes.byref(guides) if guides is not None else None, *head, ptr("denoised"), ptr("sum"),
                          ptr(noisy_name), ptr("beauty"), ctypes.byref(st), ctypes.byref(ms)))
        for name in ("denoised", noisy_name):
            if name in out:
                out[name] = out[name][:K]
        out["denoise_ms"] = ms.value
        out["guides_ms"] = self.denoise_parts_timings()["guides_ms"]
        return out

    def render_denoised_light_groups(self, p, groups, params=None, guides=None, with_sum=True, with_groups=False,
                                     with_beauty=False, stats=None, n_groups=None):
        """render_light_groups() and the group images denoised one by one with shared guides, on the device
        (nart_hip_render_denoised_light_groups): a dict with "denoised", (G, totalH, totalW, 5), image g with
        the bits of denoise() over group g and the AOVs of render_aovs(); "sum" of the denoised groups;
        "groups" and "beauty", the noisy images with render_light_groups()'s bits, if requested;
        "denoise_ms", the device time of the stage; "guides_ms", the render time of the guides frame.
        guides: a GuideParams selects the followed guides (as render_denoised).  light_mix() takes
        "denoised" as it takes "groups"."""
        m, n, G = self._light_group_map(groups)
        G = G if n_groups is None else int(n_groups)
        head = (m.ctypes.data if m is not None else None, n, G)
        return self._denoised_parts_call(p, self._lib.nart_hip_render_denoised_light_groups, head, G, "groups", params, guides,
                                         with_sum, with_groups, with_beauty, stats)

    def render_denoised_depth_layers(self, p, cuts, params=None, guides=None, with_sum=True, with_layers=False,
                                     with_beauty=False, stats=None, n_cuts=None):
        """render_depth_cuts(), depth_layers() and the K + 1 layers denoised one by one with shared guides, on
        the device (nart_hip_render_denoised_depth_layers): a dict with "denoised", (K + 1, totalH, totalW, 5);
        "sum" of the denoised layers; "layers" (the noisy layers, depth_layers()'s bits) and "beauty" if
        requested; "denoise_ms" and "guides_ms" as render_denoised_light_groups()."""
        c, K = self._depth_cut_list(cuts)
        K = K if n_cuts is None else int(n_cuts)
        head = (c.ctypes.data if c is not None else None, K)
        return self._denoised_parts_call(p, self._lib.nart_hip_render_denoised_depth_layers, head, min(K, 8) + 1, "layers",
                                         params, guides, with_sum, with_layers, with_beauty, stats)

    def denoise_parts_timings(self):
        """Device times (ms) of the last parts denoise, summed over its chunks, and the render time of the
        last whole-frame call's guides frame (nart_hip_denoise_parts_timings): {"prepare", "variance",
        "passes": [8], "finalize", "sum", "guides_ms"}."""
        v = [ctypes.c_double() for _ in range(5)]
        passes = (ctypes.c_double * 8)()
        self._check(self._lib.nart_hip_denoise_parts_timings(self._ctx, ctypes.byref(v[0]), ctypes.byref(v[1]), passes,
                                                             ctypes.byref(v[2]), ctypes.byref(v[3]), ctypes.byref(v[4])))
        return {"prepare": v[0].value, "variance": v[1].value, "passes": list(passes), "finalize": v[2].value,
                "sum": v[3].value, "guides_ms": v[4].value}

    def render_device(self, p, stats=None):
        """Whole session, image left on the (first) device: returns its device address (totalH x
        totalW x 5 float32, owned by the context until the next render).  Multi-device contexts
        gather over their RCCL send/receive group first (nart_hip_render_device)."""
        st = stats if stats is not None else RenderStats()
        ptr = _P()
        self._check(self._lib.nart_hip_render_device(self._ctx, ctypes.byref(p), ctypes.byref(ptr), ctypes.byref(st)))
        return ptr.value

    def render_buckets_async(self, p, bucket_ids, d_tiles_ptr, stream_ptr=0, stats=None):
        ids = np.ascontiguousarray(bucket_ids, dtype=np.uint32)
        st = stats if stats is not None else RenderStats()
        self._check(self._lib.nart_hip_render_buckets_async(
            self._ctx, ctypes.byref(p), ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(ids),
            _P(d_tiles_ptr), _P(stream_ptr), ctypes.byref(st)))
        return st

    def combine_async(self, p, d_tiles_ptr, d_image_ptr, stream_ptr=0):
        self._check(self._lib.nart_hip_combine_async(self._ctx, ctypes.byref(p), _P(d_tiles_ptr), _P(d_image_ptr),
                                                     _P(stream_ptr)))

    def render_samples(self, p, x0, y0, w, h):
        out = np.empty((h, w, p.spp, 4), np.float32)
        self._check(self._lib.nart_hip_render_samples(self._ctx, ctypes.byref(p), x0, y0, w, h, out.ctypes.data))
        return out

    def eval_sincos(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        s = np.empty_like(x)
        c = np.empty_like(x)
        self._check(self._lib.nart_hip_eval_sincos(self._ctx, x.ctypes.data, len(x), s.ctypes.data, c.ctypes.data))
        return s, c

    def eval(self, op, inputs, fm=None):
        """Device probe (nart_hip_eval): one device function of the render path on caller-supplied
        inputs.  op: a name or number of EVAL_OPS; inputs: (n, 16) float32 records, integer fields as
        their bits (include/nart_hip.h documents the fields per op); fm: the feature mask bxdf_f_pdf
        and bxdf_sample_f are built for (an EVAL_MASKS mask; None: FT_ALL).  Returns (n, 16) float32."""
        x = np.ascontiguousarray(inputs, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != EVAL_WORDS:
            raise ValueError("probe inputs must be (n, %d) float32 records, got %r" % (EVAL_WORDS, x.shape))
        out = np.zeros_like(x)
        self._check(self._lib.nart_hip_eval(self._ctx, EVAL_OPS[op] if isinstance(op, str) else int(op),
                                            FT_ALL if fm is None else int(fm), x.ctypes.data, len(x), out.ctypes.data))
        return out

    def trace(self, rays, variant="plain", sk=0, count=False):
        """Device trace probe (nart_hip_trace): caller-supplied rays against this context's device scene,
        answered by one of the render kernels' traversal entry points.  rays: (n, 8) float32 records
        (trace_rays builds them); variant: a name or number of TRACE_VARIANTS; sk: the STEP variants'
        LDS stack levels (0: the whole stack); count: also return the lanes' traversal counters.
        Returns (n, 32) uint32 records (include/nart_hip.h documents the words)."""
        x = np.ascontiguousarray(rays, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != TRACE_IN_WORDS:
            raise ValueError("trace rays must be (n, %d) float32 records, got %r" % (TRACE_IN_WORDS, x.shape))
        out = np.zeros((len(x), TRACE_OUT_WORDS), np.uint32)
        self._check(self._lib.nart_hip_trace(self._ctx, TRACE_VARIANTS[variant] if isinstance(variant, str) else int(variant),
                                             int(sk), 1 if count else 0, x.ctypes.data, len(x), out.ctypes.data))
        return out

    def scene_eval(self, op, records, build=None):
        """Device scene probe (nart_hip_scene_eval): one scene-bound device function (patterns, lights, BSDF
        set-up, medium) on caller-supplied records against this context's device scene.  op: a name or
        number of SCENE_OPS; records: (n, 16) float32, integer fields as their bits (include/nart_hip.h
        documents the fields per op); build: a name or number of SCENE_BUILDS (None: "env_all", the generic
        build, which every scene fits).  Returns (n, 32) float32."""
        x = np.ascontiguousarray(records, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != SCENE_IN_WORDS:
            raise ValueError("scene probe records must be (n, %d) float32, got %r" % (SCENE_IN_WORDS, x.shape))
        out = np.zeros((len(x), SCENE_OUT_WORDS), np.float32)
        b = 0 if build is None else (SCENE_BUILDS[build] if isinstance(build, str) else int(build))
        self._check(self._lib.nart_hip_scene_eval(self._ctx, SCENE_OPS[op] if isinstance(op, str) else int(op), b,
                                                  x.ctypes.data, len(x), out.ctypes.data))
        return out

    def close(self):
        if self._ctx:
            self._lib.nart_hip_destroy(self._ctx)
            self._ctx = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def finalize(p, image):
    """WriteImageToEXR's per-pixel result = contribution / filterWeightSum (render.cpp:213-222)."""
    g = session_geometry(p)
    fb = g.filter_bounds
    crop = image[fb:fb + p.image_height, fb:fb + p.image_width]
    with np.errstate(divide="ignore", invalid="ignore"):
        return crop[..., :4] / crop[..., 4:5]


def adaptive_levels(params, spp):
    """Host only: the sample counts of the adaptive levels for a maximum of spp samples
    (nart_hip_adaptive_levels): min_spp, times growth per level, ending on spp.  params an
    AdaptiveParams (None: the defaults)."""
    lib = hip_lib()
    levels, n = (ctypes.c_uint32 * 32)(), ctypes.c_uint32()
    rc = lib.nart_hip_adaptive_levels(ctypes.byref(params) if params else None, spp, levels, ctypes.byref(n))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_adaptive_levels: invalid parameters or spp < 2")
    return [int(levels[i]) for i in range(n.value)]


def matte_ids(scene, kind=MATTE_MESH):
    """Host only: the number of matte ids N of a scene for an id kind (nart_hip_matte_ids): its meshes
    (MATTE_MESH) or its materials (MATTE_MATERIAL).  More than 32 raise NART_E_UNSUPPORTED."""
    n = ctypes.c_uint32()
    rc = hip_lib().nart_hip_matte_ids(scene.blob, int(kind), ctypes.byref(n))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_matte_ids: %s" % ("an unknown id kind" if rc == -1
                                                        else "%d ids; at most 32 are supported" % n.value))
    return n.value


def cascade_levels(params=None):
    """Host only: the brightness levels b_0 .. b_{K-1} of the firefly cascade as float32
    (nart_hip_cascade_levels).  params a CascadeParams (None: the defaults); invalid ones raise."""
    lib = hip_lib()
    levels, n = (ctypes.c_float * 8)(), ctypes.c_uint32()
    rc = lib.nart_hip_cascade_levels(ctypes.byref(params) if params else None, levels, ctypes.byref(n))
    if rc != NART_OK:
        raise NartError(rc, "nart_hip_cascade_levels: invalid cascade parameters")
    return np.array([levels[i] for i in range(n.value)], np.float32)


def spp_image(p, bucket_spp):
    """The per-pixel sample count of an adaptive render: the cropped (H, W) uint32 map in which every
    pixel holds the sample count of the bucket that traced it (render_adaptive()'s "bucket_spp")."""
    g = session_geometry(p)
    b = np.ascontiguousarray(bucket_spp, np.uint32).reshape(g.n_buckets_y, g.n_buckets_x)
    B = p.bucket_size
    return np.repeat(np.repeat(b, B, axis=0), B, axis=1)[:p.image_height, :p.image_width].copy()


def half_mean(half):
    """The mean colour of a half buffer of render_halves(), normalised by the half's own weights:
    (..., 3) float32 rgb / contribution[3], and 0 where the half holds no sample."""
    h = np.ascontiguousarray(half, np.float32)
    with np.errstate(all="ignore"):
        return np.where((h[..., 3] > 0)[..., None], h[..., :3] / h[..., 3:4], np.float32(0)).astype(np.float32)


def sample_variance(p, beauty, moment):
    """The per-pixel variance image of a render, for users with their own denoiser or sampling loop:
    the cropped (H, W, 4) float32 {V.rgb, 1/k} from the beauty and the second-moment image of
    render_aovs(moment=True), by the header's formula (include/nart_hip.h, "Sample variance"), every
    operation in float32 and in its order.  With M the moment pixel, mw its filter weight sum and
    c = beauty.rgb / beauty.w (0 where beauty.w <= 0):
        k = M.a / (mw * mw)         1 / k is the pixel's effective sample count
        V.ch = max(0, M.ch / mw - c.ch * c.ch) * k      the variance of the filtered mean, no Bessel correction
    and all four are 0 where mw <= 0."""
    g = session_geometry(p)
    fb, f32 = g.filter_bounds, np.float32
    crop = lambda im: np.ascontiguousarray(im, f32)[fb:fb + p.image_height, fb:fb + p.image_width]
    B, M = crop(beauty), crop(moment)
    out = np.zeros(B.shape[:2] + (4,), f32)
    with np.errstate(all="ignore"):
        bw, mw = B[..., 4], M[..., 4]
        c = np.where((bw > 0)[..., None], B[..., :3] / bw[..., None], f32(0)).astype(f32)
        k = (M[..., 3] / (mw * mw)).astype(f32)
        m2 = (M[..., :3] / mw[..., None]).astype(f32)
        d = (m2 - c * c).astype(f32)
        var = np.where(f32(0) > d, f32(0), d).astype(f32)  # max(0, d) = 0 > d ? 0 : d
        ok = mw > 0
        out[..., :3] = np.where(ok[..., None], var * k[..., None], f32(0))
        out[..., 3] = np.where(ok, f32(1) / k, f32(0))
    return out
