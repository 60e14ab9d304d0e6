"""ctypes mirror of include/pt_api.h (the C ABI of the hot path).

Plumbing only: struct layouts, function prototypes and a thin `Library` wrapper that
binds either the product library (prefix ``pt_``, the HIP engine) or — from tests —
the CPU oracle (prefix ``ptref_``).  No computation happens here.
"""
import collections
import ctypes as C
import numpy as np

PT_OK = 0
PT_ERR_INVALID_ARGUMENT = 1
PT_ERR_UNSUPPORTED = 4   # pt_status, include/pt_api.h
TAG_MATERIAL, TAG_LIGHT, TAG_CAMERA = 0, 1, 2
MATERIAL_NONE = 0xFFFFFFFF

CURVE_LINEAR, CURVE_TABULATED, CURVE_CAUCHY, CURVE_EXPONENTIAL, CURVE_INV_EXPONENTIAL, CURVE_BLACKBODY, CURVE_CONST = range(7)
INTERP_LINEAR, INTERP_NEAREST, INTERP_CUBIC = range(3)
TEXTURE1, TEXTURE4 = 1, 4
MATERIAL_LAMBERTIAN, MATERIAL_GGX, MATERIAL_DIFFUSE_LIGHT, MATERIAL_SHARP_LIGHT, MATERIAL_PASSTHROUGH = range(5)
MEDIUM_HG, MEDIUM_RAYLEIGH = range(2)
SIDED_FORWARD, SIDED_REVERSE, SIDED_DUAL = range(3)
SHAPE_RECT, SHAPE_SPHERE, SHAPE_DISK, SHAPE_MESH = range(4)
AXIS_X, AXIS_Y, AXIS_Z = range(3)
ENV_CONSTANT, ENV_SUN, ENV_HDR = range(3)


def material_id(tag, index):
    return ((tag & 3) << 16) | (index & 0xFFFF)


class Curve(C.Structure):
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("p0", C.c_float), ("p1", C.c_float),
                ("data_offset", C.c_uint32), ("data_count", C.c_uint32)]


class TextureLayer(C.Structure):
    _fields_ = [("kind", C.c_int32), ("curves", C.c_int32 * 4), ("width", C.c_int32), ("height", C.c_int32),
                ("data_offset", C.c_uint64)]


class TexStack(C.Structure):
    _fields_ = [("first_layer", C.c_int32), ("layer_count", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("texstack", C.c_int32), ("alpha", C.c_float),
                ("curve_eta", C.c_int32), ("curve_eta_o", C.c_int32), ("curve_kappa", C.c_int32),
                ("curve_emit", C.c_int32), ("curve_bounce", C.c_int32), ("sharpness", C.c_float),
                ("sidedness", C.c_int32), ("outer_medium", C.c_int32), ("inner_medium", C.c_int32)]


class Medium(C.Structure):
    _fields_ = [("kind", C.c_int32), ("curve_g", C.c_int32), ("curve_sigma_a", C.c_int32), ("curve_sigma_s", C.c_int32),
                ("curve_ior", C.c_int32), ("corrective_factor", C.c_float)]


class Mesh(C.Structure):
    _fields_ = [("vertex_offset", C.c_uint32), ("vertex_count", C.c_uint32), ("index_offset", C.c_uint32),
                ("face_count", C.c_uint32), ("normal_offset", C.c_int32), ("face_material_offset", C.c_int32)]


class Instance(C.Structure):
    _fields_ = [("kind", C.c_int32), ("has_transform", C.c_int32), ("material", C.c_uint32), ("mesh", C.c_int32),
                ("origin", C.c_float * 3), ("size", C.c_float * 2), ("radius", C.c_float), ("axis", C.c_int32),
                ("two_sided", C.c_int32), ("forward", C.c_float * 16), ("reverse", C.c_float * 16)]


class Environment(C.Structure):
    _fields_ = [("kind", C.c_int32), ("strength", C.c_float), ("curve", C.c_int32), ("angular_diameter", C.c_float),
                ("sun_direction", C.c_float * 3), ("texstack", C.c_int32), ("rotation_forward", C.c_float * 16),
                ("rotation_reverse", C.c_float * 16), ("importance_width", C.c_int32), ("importance_height", C.c_int32),
                ("importance_luminance_curve", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("look_from", C.c_float * 3), ("look_at", C.c_float * 3), ("v_up", C.c_float * 3),
                ("vfov", C.c_float), ("focal_distance", C.c_float), ("aperture_diameter", C.c_float),
                ("kind", C.c_int32), ("fov", C.c_float * 2)]


CAMERA_PROJECTIVE, CAMERA_PANORAMA = 0, 1


class SceneDesc(C.Structure):
    _fields_ = [
        ("curve_count", C.c_uint32), ("curves", C.POINTER(Curve)),
        ("curve_data_count", C.c_size_t), ("curve_data", C.POINTER(C.c_float)),
        ("layer_count", C.c_uint32), ("layers", C.POINTER(TextureLayer)),
        ("texstack_count", C.c_uint32), ("texstacks", C.POINTER(TexStack)),
        ("texture_data_count", C.c_size_t), ("texture_data", C.POINTER(C.c_float)),
        ("material_count", C.c_uint32), ("materials", C.POINTER(Material)),
        ("mesh_count", C.c_uint32), ("meshes", C.POINTER(Mesh)),
        ("vertex_count", C.c_size_t), ("vertices", C.POINTER(C.c_float)),
        ("index_count", C.c_size_t), ("indices", C.POINTER(C.c_uint32)),
        ("normal_count", C.c_size_t), ("normals", C.POINTER(C.c_float)),
        ("face_material_count", C.c_size_t), ("face_materials", C.POINTER(C.c_uint32)),
        ("instance_count", C.c_uint32), ("instances", C.POINTER(Instance)),
        ("camera_count", C.c_uint32), ("cameras", C.POINTER(Camera)),
        ("environment", Environment),
        ("env_sampling_probability", C.c_float),
        ("medium_count", C.c_uint32), ("mediums", C.POINTER(Medium)),
    ]


class RenderDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("spp", C.c_uint32), ("min_bounces", C.c_uint32),
                ("max_bounces", C.c_uint32), ("light_samples", C.c_uint32), ("only_direct", C.c_uint32),
                ("wavelength_lo", C.c_float), ("wavelength_hi", C.c_float), ("camera_index", C.c_uint32),
                ("seed", C.c_uint64), ("tile_width", C.c_uint32), ("tile_height", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("hero_wavelengths", C.c_uint32),
                ("first_sample", C.c_uint32), ("sample_count", C.c_uint32), ("phase_samples", C.c_uint32),
                ("medium_aware", C.c_uint32)]


class AdaptiveDesc(C.Structure):
    """pt_adaptive_desc (include/pt_adaptive.h): the ceiling, the samples per round, the target error."""
    _fields_ = [("max_samples", C.c_uint32), ("step", C.c_uint32), ("rel_error", C.c_float), ("abs_error", C.c_float)]


class SpectralDesc(C.Structure):
    """pt_spectral_desc (include/pt_spectral.h): the number of wavelength bins (1..64)."""
    _fields_ = [("bins", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class LightGroupsDesc(C.Structure):
    """pt_light_groups_desc (include/pt_light_groups.h): G, one group id per instance, the environment's group."""
    _fields_ = [("group_count", C.c_uint32), ("instance_count", C.c_uint32), ("instance_group", C.POINTER(C.c_uint8)), ("environment_group", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


LIGHT_GROUPS_MAX = 8


class PathPassesDesc(C.Structure):
    """pt_path_passes_desc (include/pt_light_groups.h): reserved words, all 0."""
    _fields_ = [("reserved", C.c_uint32 * 4)]


# PT_PATH_PASSES and the PT_PATH_PASS_* indices (include/pt_light_groups.h): the order of the pass films, and their names in a file name
PATH_PASSES = 8
PATH_PASS_NAMES = ("emission", "background", "diffuse_direct", "diffuse_indirect", "reflection_direct", "reflection_indirect", "transmission_direct",
                   "transmission_indirect")


# PT_PATH_EXPRS_MAX, PT_PATH_EXPR_STATES_MAX, PT_PATH_EXPR_TERMINALS, PT_PATH_EXPR_ENVIRONMENT (include/pt_light_groups.h, "Path expressions")
PATH_EXPRS_MAX, PATH_EXPR_STATES_MAX, PATH_EXPR_TERMINALS, PATH_EXPR_ENVIRONMENT = 8, 64, 9, 8


class PathExprProgram(C.Structure):
    """pt_path_expr_program (include/pt_light_groups.h): K, the states, the start, the environment's group, 16 bytes per state — word 0 the successors behind D, R
    and T, 6 bits each; words 1..3 nine 8-bit output masks, terminal symbol s in byte s % 4 of word 1 + s // 4."""
    _fields_ = [("outputs", C.c_uint32), ("states", C.c_uint32), ("start", C.c_uint32), ("environment_group", C.c_uint32),
                ("table", C.c_uint32 * 4 * PATH_EXPR_STATES_MAX)]


# the eight path passes written as path expressions, in the order of PATH_PASS_NAMES
PATH_PASS_EXPRS = ("CL", "CE", "CD[LE]", "CD.+[LE]", "CR[LE]", "CR.+[LE]", "CT[LE]", "CT.+[LE]")


def light_group_gains(gains):
    """G scalars as the G scaled identities of a mix, float32 [G,3,3]: group g's film times gains[g]."""
    gains = np.asarray(gains, np.float32).reshape(-1)
    return (gains[:, None, None] * np.eye(3, dtype=np.float32)[None]).astype(np.float32)


# include/pt_spectral.h: a response that is no curve (a component of the engine's colour-matching fit), the absent filter, the caps of a development
RESPONSE_CIE_X, RESPONSE_CIE_Y, RESPONSE_CIE_Z = -1, -2, -3
SPECTRAL_NO_FILTER = -1
RELAMP_KEEP = -1   # PT_RELAMP_KEEP (include/pt_light_groups_spectral.h): a group keeps its lamp
SPECTRAL_MAX_RESPONSES, SPECTRAL_MAX_SUBSAMPLES = 16, 16


class DenoiseDesc(C.Structure):
    """pt_denoise_desc (include/pt_denoise.h): film size, passes, the three edge-stopping parameters (0 = default), the device."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_depth", C.c_float),
                ("normal_power_log2", C.c_uint32), ("device", C.c_uint32), ("reserved", C.c_uint32 * 1)]


# include/pt_resident.h: the parts of a scene's resident set, and pt_resident_denoise_desc's flag
RESIDENT_FILM, RESIDENT_BINS, RESIDENT_GUIDES, RESIDENT_ALBEDO, RESIDENT_BIN_ALBEDO, RESIDENT_DENOISED, RESIDENT_DENOISED_BINS = (1 << i for i in range(7))
RESIDENT_PLANAR_GATHER = 1
RESIDENT_ASSEMBLE_STAGED = 1


class ResidentInfo(C.Structure):
    """struct pt_resident_info (include/pt_resident.h): the resident set's size, bins and RESIDENT_* bits."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bins", C.c_uint32), ("parts", C.c_uint32)]


class ResidentDenoiseDesc(C.Structure):
    """pt_resident_denoise_desc (include/pt_resident.h): the filter's parameters (size 0 = the resident one; the device is ignored) and the gather's form."""
    _fields_ = [("filter", DenoiseDesc), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class GuideChainDesc(C.Structure):
    """pt_guide_chain_desc (include/pt_denoise.h): the specular vertices followed per guide sample, the GGX alpha up to which a material is specular (0 = 0.01)."""
    _fields_ = [("max_chain", C.c_uint32), ("alpha_max", C.c_float), ("reserved", C.c_uint32 * 2)]


class MatteDesc(C.Structure):
    """pt_matte_desc (include/pt_denoise.h): the camera samples per pixel, the ranks kept per pixel, what a sample is keyed by (MATTE_KEY_*)."""
    _fields_ = [("samples", C.c_uint32), ("ranks", C.c_uint32), ("key", C.c_uint32), ("reserved", C.c_uint32 * 1)]


MATTE_KEY_INSTANCE, MATTE_KEY_MATERIAL = 0, 1
MATTE_KEYS = {"instance": MATTE_KEY_INSTANCE, "material": MATTE_KEY_MATERIAL}
MATTE_SKY, MATTE_NONE = 0xFFFFFFFE, 0xFFFFFFFF   # the key of a sample that hit nothing, the key of an empty rank
MATTE_RANKS_MAX = 8


def matte_selections(selections):
    """A list of iterables of keys as pt_matte_extract takes it: (set_count, offsets [M+1] u32, selected u32)."""
    sets = [np.asarray(list(s), dtype=np.uint32).reshape(-1) for s in selections]
    offsets = np.zeros(len(sets) + 1, np.uint32)
    if sets:
        offsets[1:] = np.cumsum([s.size for s in sets])
    selected = np.concatenate(sets) if sets else np.zeros(0, np.uint32)
    return len(sets), offsets, np.ascontiguousarray(selected, dtype=np.uint32)


class Profile(C.Structure):
    _fields_ = [("bounce_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("light_rays", C.c_uint64),
                ("camera_rays", C.c_uint64), ("env_hits", C.c_uint64), ("seconds", C.c_double),
                ("kernel_seconds", C.c_double * 8), ("kernel_launches", C.c_uint64 * 8), ("stage_items", C.c_uint64 * 8)]

    def as_dict(self):
        return {"bounce_rays": self.bounce_rays, "shadow_rays": self.shadow_rays, "light_rays": self.light_rays,
                "camera_rays": self.camera_rays, "env_hits": self.env_hits, "seconds": self.seconds,
                "kernel_seconds": list(self.kernel_seconds), "kernel_launches": list(self.kernel_launches), "stage_items": list(self.stage_items)}


# pt_tuning flags (include/pt_api.h)
TUNE_NO_LDS, TUNE_NO_CORE_LDS, TUNE_NO_PARK, TUNE_NO_LIVE_LIST, TUNE_EXACT_SLAB, TUNE_NO_CULL, TUNE_NO_SWEEP, TUNE_NO_MESH_SWEEP, TUNE_NO_KNOWN_LIGHT, \
    TUNE_GENERAL_FORMS, TUNE_NO_FUSE, TUNE_NO_STAGE_TIMING, TUNE_MULTI_RCCL, TUNE_NO_AXIS_SCAN, TUNE_NO_ONE_LIGHT, TUNE_NO_CONVEX, TUNE_NO_MESH_SHORTCUTS, \
    TUNE_NO_PASS_OVERLAP = (1 << i for i in range(18))
TUNE_PASS_SKEW_SHIFT, TUNE_PASS_SKEW_MASK = 18, 7   # flags bits 18..20: 0 = the default skew, 1 = none, 2 + g = behind bounce g


class Tuning(C.Structure):
    """pt_tuning: the engine's run-time switches, taken by a scene when it is created."""
    _fields_ = [("flags", C.c_uint32), ("batch_slots", C.c_uint32), ("blocks_per_cu", C.c_uint32), ("park_blocks_per_cu", C.c_uint32),
                ("park_dynamic", C.c_int32), ("shade_form", C.c_uint32), ("lds_all_limit", C.c_uint32), ("multi_virtual", C.c_uint32),
                ("walk_evict_below", C.c_uint32), ("walk_search_below", C.c_uint32), ("park_block", C.c_uint32), ("light_prepass_max", C.c_uint32), ("top_evict_below", C.c_uint32), ("group_evict_below", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class OutputDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tonemap", C.c_int32), ("luminance_only", C.c_int32),
                ("exposure", C.c_float), ("key_value", C.c_float), ("white_point", C.c_float), ("colorspace", C.c_int32),
                ("factor", C.c_float)]


TONEMAP_CLAMP, TONEMAP_REINHARD0, TONEMAP_REINHARD1 = range(3)
COLORSPACE_SRGB, COLORSPACE_REC709, COLORSPACE_REC2020 = range(3)
COMPARE_ABSOLUTE, COMPARE_RMSE, COMPARE_RELATIVE = range(3)


class CompareStats(C.Structure):
    _fields_ = [("linf", C.c_double * 4), ("mean_abs", C.c_double * 4), ("rmse", C.c_double), ("pixel_min", C.c_float),
                ("pixel_max", C.c_float), ("nonfinite", C.c_uint64)]

    def as_dict(self):
        return {"linf": list(self.linf), "mean_abs": list(self.mean_abs), "rmse": self.rmse, "pixel_min": self.pixel_min,
                "pixel_max": self.pixel_max, "nonfinite": int(self.nonfinite)}


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("point", C.c_float * 3), ("normal", C.c_float * 3), ("uv", C.c_float * 2),
                ("material", C.c_uint32), ("instance", C.c_uint32), ("valid", C.c_int32)]


HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", 3), ("normal", "<f4", 3), ("uv", "<f4", 2),
                      ("material", "<u4"), ("instance", "<u4"), ("valid", "<i4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit)

# every entry point include/pt_api.h declares (without prefix)
API_FUNCTIONS = ["scene_create", "scene_create_tuned", "tuning_default", "scene_destroy", "last_error", "render", "render_device", "render_multi", "device_count", "intersect",
                 "bsdf_sample", "bsdf_eval", "emission", "curve_eval", "camera_samples", "device_info", "output_film", "write_png", "write_exr", "compare_films"]


class PtError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("pt_status %d: %s" % (status, message))
        self.status = status


def _pointer_to(ctype):
    """array -> its data as a pointer to `ctype`; None (an output not asked for, an input not given) stays None."""
    pointer = C.POINTER(ctype)
    return lambda a: None if a is None else a.ctypes.data_as(pointer)


_fp, _u32p, _u8p, _f64p = (_pointer_to(t) for t in (C.c_float, C.c_uint32, C.c_uint8, C.c_double))


def render_desc(width, height, spp, max_bounces, min_bounces=1, light_samples=2, only_direct=False,
                wavelength=(380.0, 750.0), camera_index=0, seed=1, tile=(32, 32), shard=(0, 0),
                hero_wavelengths=1, first_sample=0, sample_count=0, phase_samples=0, medium_aware=False):
    return RenderDesc(width, height, spp, min_bounces, max_bounces, light_samples, int(bool(only_direct)),
                      wavelength[0], wavelength[1], camera_index, seed, tile[0], tile[1], shard[0], shard[1],
                      hero_wavelengths, first_sample, sample_count, phase_samples, int(bool(medium_aware)))


# One row per entry of the boundary (without prefix).  `required`: a library without the entry does not load (unless Library's `optional` names it); any
# other missing entry binds as None.  `channel`: the *_last_error entry an emulation library reports this entry's refusals through — the engine, and a
# library without that channel, report through last_error.  The channels are rows like any other.
Entry = collections.namedtuple("Entry", "name argtypes restype required channel", defaults=(C.c_int32, False, None))

_P = C.POINTER
_vp, _str, _sz, _u32, _i32, _u64 = C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_uint64
_f32s, _u32s, _f64s, _u8s, _i32s = _P(C.c_float), _P(C.c_uint32), _P(C.c_double), _P(C.c_uint8), _P(C.c_int32)
_RD, _AD, _SD, _GD, _DD, _RDD, _CHAIN, _PROF, _PD = (_P(t) for t in (RenderDesc, AdaptiveDesc, SpectralDesc, LightGroupsDesc, DenoiseDesc, ResidentDenoiseDesc,
                                                                     GuideChainDesc, Profile, PathPassesDesc))
_PX = _P(PathExprProgram)
_DENOISE, _ALBEDO, _BIN_ALBEDO, _PROJECT = "denoise_last_error", "denoise_albedo_last_error", "denoise_spectral_albedo_last_error", "spectral_project_last_error"
_GROUPS, _GROUP_BINS, _RESIDENT = "light_groups_last_error", "light_groups_spectral_last_error", "resident_last_error"

BINDINGS = (
    ("pt_api.h", (
        Entry("scene_create", [_P(SceneDesc), _P(_vp)], required=True),
        Entry("scene_create_tuned", [_P(SceneDesc), _P(Tuning), _P(_vp)]),
        Entry("tuning_default", [_P(Tuning)], None),
        Entry("scene_destroy", [_vp], None, required=True),
        Entry("last_error", [], _str, required=True),
        Entry("render", [_vp, _RD, _f32s, _PROF], required=True),
        Entry("render_device", [_vp, _RD, _vp, _vp, _PROF]),
        Entry("render_multi", [_vp, _RD, _u64, _f32s, _PROF]),
        Entry("device_count", [], _u32),
        Entry("intersect", [_vp, _sz, _f32s, _f32s, _P(Hit)], required=True),
        Entry("camera_samples", [_vp, _RD, _sz, _u32s, _u32s, _f32s, _f32s, _f32s], required=True),
        Entry("bsdf_sample", [_vp, _u32, _sz, _f32s, _f32s, _f32s, _f32s, _f32s, _f32s], required=True),
        Entry("bsdf_eval", [_vp, _u32, _sz, _f32s, _f32s, _f32s, _f32s, _f32s], required=True),
        Entry("emission", [_vp, _u32, _sz, _f32s, _f32s, _f32s], required=True),
        Entry("curve_eval", [_vp, _u32, _sz, _f32s, _f32s], required=True),
        Entry("device_info", [], _str),
        Entry("output_film", [_P(OutputDesc), _f32s, _u8s, _f32s]),
        Entry("write_png", [_str, _u32, _u32, _u8s, _i32]),
        Entry("compare_films", [_u32, _u32, _f32s, _f32s, _i32, _f32s, _P(CompareStats)]),
        Entry("write_exr", [_str, _u32, _u32, _f32s, _i32]))),
    # not the oracle's boundary: the reference cannot sample an emissive mesh face (debug_scene_info is the engine's, declared in no public header)
    ("pt_debug.h", (
        Entry("light_sample", [_vp, _u32, _sz, _f32s, _f32s, _f32s, _f32s]),
        Entry("debug_scene_info", [_vp, _i32], _u32))),
    # not the oracle's boundary either: the reference's tiled renderer has no adaptive sampling
    ("pt_adaptive.h", (
        Entry("render_adaptive", [_vp, _RD, _AD, _f32s, _u32s, _f64s, _PROF]),
        Entry("render_adaptive_multi", [_vp, _RD, _AD, _u64, _f32s, _u32s, _f64s, _PROF]))),
    # the reference has no denoiser; the oracle and older emulation libraries do not export these
    ("pt_denoise.h", (
        Entry("render_guides", [_vp, _RD, _u32, _f32s], channel=_DENOISE),
        Entry("denoise_film", [_DD, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s], channel=_DENOISE),
        Entry(_DENOISE, [], _str),
        Entry("albedo_basis", [_RD, _f32s, _f32s], channel=_ALBEDO),
        Entry("render_guides_albedo", [_vp, _RD, _u32, _f32s, _f32s], channel=_ALBEDO),
        Entry("denoise_film_albedo", [_DD, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s, _f32s], channel=_ALBEDO),
        Entry(_ALBEDO, [], _str),
        Entry("render_guides_chain", [_vp, _RD, _u32, _CHAIN, _f32s, _f32s], channel="guides_chain_last_error"),
        Entry("guides_chain_last_error", [], _str),
        Entry("render_mattes", [_vp, _RD, _P(MatteDesc), _u32s, _f32s, _u32s], channel=_DENOISE),
        Entry("mattes_resident", [_vp, _u32s, _u32s, _u32s, _u32s], channel=_DENOISE),
        Entry("matte_extract", [_u32, _u32, _u32, _u32s, _f32s, _u32, _u32s, _u32s, _u32, _f32s], channel=_DENOISE),
        Entry("matte_extract_resident", [_vp, _u32, _u32s, _u32s, _f32s], channel=_DENOISE),
        Entry("cryptomatte_hash", [_str, _u32s, _f32s], channel=_DENOISE),
        Entry("write_exr_cryptomatte", [_str, _u32, _u32, _u32, _u32s, _f32s, _str, _u32, _u32s, _P(_str), _f32s, _i32]))),
    # the reference keeps no spectrum; an older library without these entries still loads
    ("pt_spectral.h", (
        Entry("render_spectral", [_vp, _RD, _SD, _f32s, _f32s, _PROF]),
        Entry("spectral_bin_centres", [_RD, _SD, _f32s]),
        Entry("write_exr_spectral", [_str, _u32, _u32, _u32, _f32s, _f32s, _f32s, _i32]),
        Entry("render_adaptive_spectral", [_vp, _RD, _AD, _SD, _f32s, _u32s, _f64s, _f32s, _PROF]),
        Entry("render_spectral_multi", [_vp, _RD, _SD, _u64, _f32s, _f32s, _PROF]),
        Entry("render_adaptive_spectral_multi", [_vp, _RD, _AD, _SD, _u64, _f32s, _u32s, _f64s, _f32s, _PROF]),
        Entry("denoise_spectral", [_DD, _u32, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s, _f32s, _f32s], channel="denoise_spectral_last_error"),
        Entry("denoise_spectral_last_error", [], _str),
        Entry("render_guides_bin_albedo", [_vp, _RD, _u32, _CHAIN, _u32, _f32s, _f32s, _f32s], channel=_BIN_ALBEDO),
        Entry("denoise_spectral_albedo", [_DD, _u32, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s, _f32s, _f32s, _f32s, _f32s], channel=_BIN_ALBEDO),
        Entry(_BIN_ALBEDO, [], _str),
        Entry("spectral_response_matrix", [_RD, _SD, _P(Curve), _u32, _f32s, _u32, _u32, _i32s, _i32, _u32, _f32s], channel=_PROJECT),
        Entry("spectral_project", [_u32, _u32, _u32, _u32, _f32s, _f32s, _f32s], channel=_PROJECT),
        Entry("spectral_project_resident", [_vp, _u32, _f32s, _f32s]),
        Entry("spectral_resident", [_vp, _u32s, _u32s, _u32s]),
        Entry(_PROJECT, [], _str))),
    # the reference keeps one film
    ("pt_light_groups.h", (
        Entry("render_light_groups", [_vp, _RD, _GD, _f32s, _f32s, _PROF], channel=_GROUPS),
        Entry("light_groups_mix", [_u32, _u32, _u32, _f32s, _f32s, _f32s], channel=_GROUPS),
        Entry("light_groups_resident", [_vp, _u32s, _u32s, _u32s], channel=_GROUPS),
        Entry("light_groups_mix_resident", [_vp, _f32s, _f32s], channel=_GROUPS),
        Entry("render_path_passes", [_vp, _RD, _PD, _f32s, _f32s, _PROF], channel=_GROUPS),
        Entry("path_expr_compile", [_P(_str), _u32, _u32, _PX, _str, _sz]),
        Entry("path_expr_match", [_PX, _str, _u32s]),
        Entry("render_path_exprs", [_vp, _RD, _PX, _u8s, _u32, _f32s, _f32s, _PROF], channel=_GROUPS),
        Entry(_GROUPS, [], _str))),
    ("pt_light_groups_spectral.h", (
        Entry("render_light_groups_spectral", [_vp, _RD, _GD, _SD, _f32s, _f32s, _f32s, _f32s, _PROF], channel=_GROUP_BINS),
        Entry("light_groups_spectral_resident", [_vp, _u32s, _u32s, _u32s, _u32s], channel=_GROUP_BINS),
        Entry("light_groups_relamp_matrix", [_RD, _SD, _P(Curve), _u32, _f32s, _u32, _u32, _i32s, _i32, _u32, _u32, _i32s, _i32s, _f32s, _f32s], channel=_GROUP_BINS),
        Entry("light_groups_relamp", [_u32, _u32, _u32, _u32, _u32, _f32s, _f32s, _f32s], channel=_GROUP_BINS),
        Entry("light_groups_relamp_resident", [_vp, _u32, _f32s, _f32s], channel=_GROUP_BINS),
        Entry(_GROUP_BINS, [], _str))),
    ("pt_light_groups_denoise.h", (
        Entry("render_adaptive_light_groups", [_vp, _RD, _AD, _GD, _f32s, _u32s, _f64s, _f32s, _PROF], channel="adaptive_light_groups_last_error"),
        Entry("denoise_light_groups", [_DD, _u32, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s, _f32s, _f32s, _f32s], channel="denoise_light_groups_last_error"),
        Entry("denoise_light_groups_resident", [_vp, _RDD, _f32s, _f32s, _f32s]),
        Entry("light_groups_denoised_resident", [_vp, _u32s, _u32s, _u32s]),
        Entry("light_groups_mix_resident_denoised", [_vp, _f32s, _f32s], channel=_GROUPS),
        Entry("render_adaptive_path_passes", [_vp, _RD, _AD, _PD, _f32s, _u32s, _f64s, _f32s, _PROF]),
        Entry("render_adaptive_path_exprs", [_vp, _RD, _AD, _PX, _u8s, _u32, _f32s, _u32s, _f64s, _f32s, _PROF]),
        Entry("adaptive_light_groups_last_error", [], _str),
        Entry("denoise_light_groups_last_error", [], _str))),
    ("pt_light_groups_multi.h", (
        Entry("render_light_groups_multi", [_vp, _RD, _GD, _u64, _f32s, _f32s, _PROF], channel=_GROUPS),
        Entry("render_adaptive_light_groups_multi", [_vp, _RD, _AD, _GD, _u64, _f32s, _u32s, _f64s, _f32s, _PROF]))),
    # an emulation library may lack these
    ("pt_resident.h", (
        Entry("resident_info", [_vp, _P(ResidentInfo)], channel=_RESIDENT),
        Entry("resident_guides", [_vp, _RD, _u32, _CHAIN, _u32], channel=_RESIDENT),
        Entry("resident_load", [_vp, _u32, _u32, _u32, _f32s, _u32s, _f64s, _f32s, _f32s, _f32s, _f32s], channel=_RESIDENT),
        Entry("denoise_resident", [_vp, _RDD, _f32s, _f32s, _f32s], channel=_RESIDENT),
        Entry("spectral_project_resident_denoised", [_vp, _u32, _f32s, _f32s], channel=_RESIDENT),
        Entry("resident_assemble", [_vp, _u32], channel=_RESIDENT),
        Entry("resident_read", [_vp, _f32s, _u32s, _f64s, _f32s], channel=_RESIDENT),
        Entry(_RESIDENT, [], _str))),
)
ENTRIES = {e.name: e for _, rows in BINDINGS for e in rows}

_BINS_LAYOUT, _GROUPS_LAYOUT = ("spectral [B,H,W]", ()), ("group_films [G,H,W,4]", (4,))   # a host-array filter's planes: their name in a refusal, a plane's trailing shape


def _filter_inputs(film, counts, stats, guides, planes=None, layout=None, albedo=None, bin_albedo=None):
    """The inputs of a host-array filter as contiguous arrays of the entry's types, refused unless all are of the film's size:
    (h, w, film, counts, stats, guides, planes, albedo, bin_albedo).  `planes` with `layout`: the spectral film or the group films."""
    film = np.ascontiguousarray(film, dtype=np.float32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    stats = np.ascontiguousarray(stats, dtype=np.float64)
    guides = np.ascontiguousarray(guides, dtype=np.float32)
    h, w = film.shape[:2]
    ok = film.shape == (h, w, 4) and counts.shape == (h, w) and stats.shape == (h, w, 2) and guides.shape == (h, w, 4)
    if layout is not None:
        planes = np.ascontiguousarray(planes, dtype=np.float32)
        ok = ok and planes.ndim == 3 + len(layout[1]) and planes.shape[1:] == (h, w) + layout[1]
    if not ok:
        raise ValueError("film [H,W,4], counts [H,W], stats [H,W,2]%s guides [H,W,4]%s of one film size" % ((",", " and " + layout[0]) if layout else (" and", "")))
    if albedo is not None:
        albedo = np.ascontiguousarray(albedo, dtype=np.float32)
        if albedo.shape != (h, w, 4):
            raise ValueError("albedo [H,W,4] of the film's size")
    if bin_albedo is not None:
        bin_albedo = np.ascontiguousarray(bin_albedo, dtype=np.float32)
        if bin_albedo.shape != (planes.shape[0], h, w):
            raise ValueError("bin_albedo [B,H,W] of the spectral film's size")
    return h, w, film, counts, stats, guides, planes, albedo, bin_albedo


def _filter_outputs(h, w, variance, planes=None):
    """(denoised film, variance or None, denoised planes or None) for a host-array filter over a film of h x w."""
    return np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32) if variance else None, None if planes is None else np.zeros(planes.shape, np.float32)


def _asked(*arrays):
    """The tuple of what was asked for: one array when one is asked for, None when none is."""
    got = tuple(a for a in arrays if a is not None)
    return got[0] if len(got) == 1 else (got or None)


def _first_device(mask):
    """The lowest device of a mask; 0 for the mask 0 (= all devices)."""
    return (mask & -mask).bit_length() - 1 if mask else 0


class Library:
    """Binds one implementation of the boundary.  `prefix` is ``pt_`` (product) or ``ptref_`` (oracle)."""

    def __init__(self, path, prefix="pt_", optional=()):
        self.path = path
        self.prefix = prefix
        self.lib = C.CDLL(path)
        for e in ENTRIES.values():
            try:
                fn = getattr(self.lib, prefix + e.name)
            except AttributeError:
                if e.required and e.name not in optional:
                    raise
                fn = None
            else:
                fn.restype, fn.argtypes = e.restype, e.argtypes
            setattr(self, "_" + e.name, fn)

    def last_error(self):
        m = self._last_error()
        return m.decode() if m else ""

    def check(self, status):
        if status != PT_OK:
            raise PtError(status, self.last_error())

    def entry(self, name):
        """The bound entry `name`; a library that lacks it is refused here."""
        fn = getattr(self, "_" + name)
        if fn is None:
            raise PtError(PT_ERR_UNSUPPORTED, "%s has no %s%s entry" % (self.path, self.prefix, name))
        return fn

    def call(self, name, *args):
        """The one way into a status-returning entry: refused if the library lacks it; a status other than PT_OK raises PtError with the message of the
        entry's own channel (ENTRIES) if the library exports that, else last_error's."""
        status = self.entry(name)(*args)
        if status != PT_OK:
            channel = ENTRIES[name].channel
            err = getattr(self, "_" + channel) if channel else None
            raise PtError(status, err().decode() if err else self.last_error())

    def device_info(self):
        return self._device_info().decode() if self._device_info else "cpu oracle"

    def path_expr_compile(self, exprs, environment_group=0):
        """pt_path_expr_compile (host only): the PathExprProgram of one expression or a sequence of up to PATH_EXPRS_MAX, expression e tagged with bit e.  A
        syntax error (PT_ERR_INVALID_ARGUMENT, "expression <e>, column <c>: ...") and more than PATH_EXPR_STATES_MAX states (PT_ERR_UNSUPPORTED) raise PtError
        with the compiler's own message."""
        exprs = [exprs] if isinstance(exprs, str) else list(exprs)
        texts = (C.c_char_p * max(len(exprs), 1))(*[e.encode() for e in exprs])
        program, err = PathExprProgram(), C.create_string_buffer(512)
        status = self.entry("path_expr_compile")(texts, len(exprs), int(environment_group), C.byref(program), err, len(err))
        if status != PT_OK:
            raise PtError(status, err.value.decode())
        return program

    def path_expr_match(self, program, path):
        """pt_path_expr_match (host only): the mask of the program's expressions that match the written-out path, such as "CDTL3" or "CRE"."""
        mask = C.c_uint32()
        status = self.entry("path_expr_match")(C.byref(program), path.encode(), C.byref(mask))
        if status != PT_OK:
            raise PtError(status, "path_expr_match: a malformed path %r or program" % (path,))
        return mask.value

    def create_scene(self, builder, tuning=None):
        """`tuning`: a Tuning (pt_scene_create_tuned); None = pt_scene_create, which reads the PT_AMD_* environment once."""
        return Scene(self, builder, tuning)

    def tuning_default(self):
        t = Tuning()
        if self._tuning_default is None:
            raise PtError(PT_ERR_UNSUPPORTED, "this library does not export %stuning_default (pt_tuning is the HIP engine's)" % self.prefix)
        self._tuning_default(C.byref(t))
        return t

    def output_film(self, film, tonemap=TONEMAP_CLAMP, luminance_only=True, exposure=0.0, key_value=0.18, white_point=1.0,
                    colorspace=COLORSPACE_SRGB, factor=1.0, want_linear=True):
        """output_film (src/renderer/mod.rs:24-80) without the file writes: (rgba8 [H,W,4] u8, linear_rgb [H,W,3] f32)."""
        film = np.ascontiguousarray(film, dtype=np.float32)
        h, w = film.shape[:2]
        d = OutputDesc(w, h, tonemap, int(bool(luminance_only)), exposure, key_value, white_point, colorspace, factor)
        rgba = np.zeros((h, w, 4), np.uint8)
        lin = np.zeros((h, w, 3), np.float32) if want_linear else None
        self.call("output_film", C.byref(d), _fp(film), _u8p(rgba), _fp(lin))
        return rgba, lin

    def compare_films(self, image, truth, mode=COMPARE_ABSOLUTE, want_image=True):
        """compare_exr (src/bin/compare_exr.rs:70-170) on raw [H,W,4] f32 images: (difference image or None, CompareStats)."""
        image = np.ascontiguousarray(image, dtype=np.float32)
        truth = np.ascontiguousarray(truth, dtype=np.float32)
        if image.shape != truth.shape or image.ndim != 3 or image.shape[2] != 4:
            raise ValueError("image dimensions must match ([H, W, 4] each)")  # the reference asserts (compare_exr.rs:66-69)
        h, w = image.shape[:2]
        out = np.zeros((h, w, 4), np.float32) if want_image else None
        st = CompareStats()
        self.call("compare_films", w, h, _fp(image), _fp(truth), mode, _fp(out), C.byref(st))
        return out, st

    def albedo_basis(self, rd):
        """pt_albedo_basis: the wavelengths [16] (nm) and the X, Y, Z weights [3,16] the albedo of a render `rd` is folded over."""
        lam, xyz = np.zeros(16, np.float32), np.zeros((3, 16), np.float32)
        self.call("albedo_basis", C.byref(rd), _fp(lam), _fp(xyz))
        return lam, xyz

    def denoise_film(self, film, counts, stats, guides, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, device=0, variance=False, albedo=None):
        """pt_denoise_film: the edge-avoiding filter over an adaptive render's film [H,W,4], counts [H,W] u32 and stats [H,W,2] f64 with the guides
        [H,W,4] of Scene.render_guides.  0 selects a parameter's default.  Returns the filtered film [H,W,4], with variance=True (film, variance [H,W]).
        `albedo` [H,W,4] (Scene.render_guides_albedo's): pt_denoise_film_albedo, the filter over the film demodulated by it."""
        name = "denoise_film" if albedo is None else "denoise_film_albedo"
        self.entry(name)
        h, w, film, counts, stats, guides, _, albedo, _ = _filter_inputs(film, counts, stats, guides, albedo=albedo)
        d = DenoiseDesc(w, h, iterations, sigma_luminance, sigma_depth, normal_power_log2, device)
        out, var, _ = _filter_outputs(h, w, variance)
        planes = [_fp(guides)] if albedo is None else [_fp(guides), _fp(albedo)]
        self.call(name, C.byref(d), _fp(film), _u32p(counts), _f64p(stats), *planes, _fp(out), _fp(var))
        return (out, var) if variance else out

    def denoise_spectral(self, film, counts, stats, guides, spectral, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, device=0, variance=False,
                         albedo=None):
        """pt_denoise_spectral: denoise_film's filter over the film and, with the same taps and weights, over the bins spectral [B,H,W] of
        Scene.render_adaptive_spectral.  Returns (denoised [H,W,4], denoised_spectral [B,H,W]), with variance=True (denoised, denoised_spectral, variance [H,W]).
        This entry has no albedo form: an `albedo` is refused (demodulating the bins needs a per-bin albedo: denoise_spectral_albedo takes both)."""
        if albedo is not None:
            raise PtError(PT_ERR_UNSUPPORTED, "denoise_spectral takes no albedo: demodulating the bins needs a per-bin albedo (denoise_spectral_albedo takes one)")
        self.entry("denoise_spectral")
        h, w, film, counts, stats, guides, spectral, _, _ = _filter_inputs(film, counts, stats, guides, spectral, _BINS_LAYOUT)
        d = DenoiseDesc(w, h, iterations, sigma_luminance, sigma_depth, normal_power_log2, device)
        out, var, out_spectral = _filter_outputs(h, w, variance, spectral)
        self.call("denoise_spectral", C.byref(d), spectral.shape[0], _fp(film), _u32p(counts), _f64p(stats), _fp(guides), _fp(spectral), _fp(out), _fp(out_spectral), _fp(var))
        return (out, out_spectral, var) if variance else (out, out_spectral)

    def denoise_spectral_albedo(self, film, counts, stats, guides, spectral, albedo=None, bin_albedo=None, iterations=0, sigma_luminance=0.0, sigma_depth=0.0,
                                normal_power_log2=0, device=0, variance=False):
        """pt_denoise_spectral_albedo: denoise_spectral over the film demodulated by `albedo` [H,W,4] (as denoise_film(albedo=...) does it) and the bins
        demodulated by `bin_albedo` [B,H,W] (Scene.render_guides_bin_albedo's); either may be None.  Returns what denoise_spectral returns."""
        self.entry("denoise_spectral_albedo")
        h, w, film, counts, stats, guides, spectral, albedo, bin_albedo = _filter_inputs(film, counts, stats, guides, spectral, _BINS_LAYOUT, albedo, bin_albedo)
        d = DenoiseDesc(w, h, iterations, sigma_luminance, sigma_depth, normal_power_log2, device)
        out, var, out_spectral = _filter_outputs(h, w, variance, spectral)
        self.call("denoise_spectral_albedo", C.byref(d), spectral.shape[0], _fp(film), _u32p(counts), _f64p(stats), _fp(guides), _fp(albedo), _fp(spectral), _fp(bin_albedo),
                  _fp(out), _fp(out_spectral), _fp(var))
        return (out, out_spectral, var) if variance else (out, out_spectral)

    def write_png(self, path, rgba8, colorspace=COLORSPACE_SRGB):
        rgba8 = np.ascontiguousarray(rgba8, np.uint8)
        self.call("write_png", path.encode(), rgba8.shape[1], rgba8.shape[0], _u8p(rgba8), colorspace)

    def write_exr(self, path, linear_rgb, colorspace=COLORSPACE_SRGB):
        linear_rgb = np.ascontiguousarray(linear_rgb, np.float32)
        self.call("write_exr", path.encode(), linear_rgb.shape[1], linear_rgb.shape[0], _fp(linear_rgb), colorspace)

    def spectral_bin_centres(self, rd, bins):
        """pt_spectral_bin_centres: the centre wavelengths [bins] (nm) of the bins of a spectral render of `rd`."""
        self.entry("spectral_bin_centres")
        centres = np.zeros(max(int(bins), 0), np.float32)
        sd = SpectralDesc(bins)
        self.call("spectral_bin_centres", C.byref(rd), C.byref(sd), _fp(centres))
        return centres

    def write_exr_spectral(self, path, centres_nm, spectral, linear_rgb=None, colorspace=COLORSPACE_SRGB):
        """pt_write_exr_spectral: spectral [bins,H,W] as one FLOAT channel per bin (S0.<centre>nm), with R, G, B from linear_rgb [H,W,3] if given."""
        self.entry("write_exr_spectral")
        spectral = np.ascontiguousarray(spectral, np.float32)
        centres_nm = np.ascontiguousarray(centres_nm, np.float32)
        if spectral.ndim != 3 or centres_nm.shape != (spectral.shape[0],):
            raise ValueError("spectral [bins, H, W] and centres_nm [bins]")
        bins, h, w = spectral.shape
        if linear_rgb is not None:
            linear_rgb = np.ascontiguousarray(linear_rgb, np.float32)
            if linear_rgb.shape != (h, w, 3):
                raise ValueError("linear_rgb [H, W, 3] of the spectral film's size")
        self.call("write_exr_spectral", path.encode(), w, h, bins, _fp(centres_nm), _fp(spectral), _fp(linear_rgb), colorspace)

    def matte_extract(self, keys, coverage, selections, device=0):
        """pt_matte_extract: the ranks keys [R,H,W] u32 and coverage [R,H,W] f32 of Scene.render_mattes and `selections`, a list of M iterables of keys (any
        order, MATTE_SKY allowed, empty allowed): float32 [M,H,W], plane m the f32 fold, over the ranks ascending, of the coverage of the ranks whose key is
        in selection m."""
        self.entry("matte_extract")
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        coverage = np.ascontiguousarray(coverage, dtype=np.float32)
        if keys.ndim != 3 or coverage.shape != keys.shape:
            raise ValueError("keys [R,H,W] and coverage [R,H,W]")
        ranks, h, w = keys.shape
        M, offsets, selected = matte_selections(selections)
        out = np.zeros((M, h, w), np.float32)
        self.call("matte_extract", w, h, ranks, _u32p(keys), _fp(coverage), M, _u32p(offsets), _u32p(selected), device, _fp(out))
        return out

    def cryptomatte_hash(self, name):
        """pt_cryptomatte_hash: (hash, id) of a name — MurmurHash3_x86_32 of its UTF-8 bytes, and the float32 whose bits are the hash made a normal number."""
        h, i = np.zeros(1, np.uint32), np.zeros(1, np.float32)
        self.call("cryptomatte_hash", name.encode(), _u32p(h), _fp(i))
        return int(h[0]), i[0]

    def write_exr_cryptomatte(self, path, keys, coverage, layer, names=None, linear_rgb=None, colorspace=COLORSPACE_SRGB):
        """pt_write_exr_cryptomatte: keys, coverage [R,H,W] as the channels <layer>NN.R/.G/.B/.A of a Cryptomatte file, with R, G, B from linear_rgb [H,W,3] if
        given.  `names`: a mapping key -> name, or a sequence of (key, name) — the manifest's entries, in this order; a key without one is named key<decimal>."""
        self.entry("write_exr_cryptomatte")
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        coverage = np.ascontiguousarray(coverage, dtype=np.float32)
        if keys.ndim != 3 or coverage.shape != keys.shape:
            raise ValueError("keys [R,H,W] and coverage [R,H,W]")
        ranks, h, w = keys.shape
        if linear_rgb is not None:
            linear_rgb = np.ascontiguousarray(linear_rgb, np.float32)
            if linear_rgb.shape != (h, w, 3):
                raise ValueError("linear_rgb [H, W, 3] of the matte's size")
        pairs = list(names.items()) if hasattr(names, "items") else list(names or [])
        name_keys = np.asarray([k for k, _ in pairs], dtype=np.uint32).reshape(-1)
        carr = (C.c_char_p * max(len(pairs), 1))(*[n.encode() for _, n in pairs])
        self.call("write_exr_cryptomatte", path.encode(), w, h, ranks, _u32p(keys), _fp(coverage), layer.encode(), len(pairs), _u32p(name_keys) if pairs else None,
                  carr if pairs else None, _fp(linear_rgb), colorspace)

    def spectral_response_matrix(self, rd, bins, responses, curves=None, curve_data=None, filter=None, subsamples=1):
        """pt_spectral_response_matrix: float32 [K, bins], row k the response responses[k] — an index into `curves` (a sequence of api.Curve whose data_offset
        points into `curve_data`, as in a scene description) or RESPONSE_CIE_X / _Y / _Z — integrated over each of the `bins` bins of a render `rd` with
        `subsamples` samples per bin, behind the curve `filter` (an index into `curves`) if one is given.  Host only."""
        self.entry("spectral_response_matrix")
        responses = [int(r) for r in responses]
        K = len(responses)
        curves = list(curves) if curves is not None else []
        carr = (Curve * max(len(curves), 1))(*curves)
        cd = np.ascontiguousarray(curve_data if curve_data is not None else [], dtype=np.float32).ravel()
        rarr = (C.c_int32 * max(K, 1))(*responses)
        matrix = np.zeros((K, max(int(bins), 0)), np.float32)
        sd = SpectralDesc(bins)
        self.call("spectral_response_matrix", C.byref(rd), C.byref(sd), carr if curves else None, len(curves), _fp(cd) if cd.size else None, cd.size, K, rarr,
                  SPECTRAL_NO_FILTER if filter is None else int(filter), subsamples, _fp(matrix))
        return matrix

    def spectral_observer_matrix(self, rd, bins, subsamples=1):
        """The three rows of the engine's colour-matching fit, float32 [3, bins]: developing a spectral film with them estimates the XYZ film."""
        return self.spectral_response_matrix(rd, bins, (RESPONSE_CIE_X, RESPONSE_CIE_Y, RESPONSE_CIE_Z), subsamples=subsamples)

    def spectral_project(self, spectral, matrix):
        """pt_spectral_project: spectral [B,H,W] projected onto the rows of matrix [K,B]: float32 [K,H,W], out[k] = the f32 fold of matrix[k,b] * spectral[b]
        over b ascending."""
        self.entry("spectral_project")
        spectral = np.ascontiguousarray(spectral, dtype=np.float32)
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if spectral.ndim != 3 or matrix.ndim != 2 or matrix.shape[1] != spectral.shape[0]:
            raise ValueError("spectral [B,H,W] and matrix [K,B]")
        bins, h, w = spectral.shape
        K = matrix.shape[0]
        out = np.zeros((K, h, w), np.float32)
        self.call("spectral_project", w, h, bins, K, _fp(matrix), _fp(spectral), _fp(out))
        return out

    def light_groups_mix(self, group_films, matrices):
        """pt_light_groups_mix: group_films [G,H,W,4] mixed by matrices [G,3,3] (light_group_gains makes them from scalars): float32 [H,W,4], per channel the f32
        fold over g ascending of acc + ((m[g,c,0] * X_g + m[g,c,1] * Y_g) + m[g,c,2] * Z_g); w = 0."""
        self.entry("light_groups_mix")
        group_films = np.ascontiguousarray(group_films, dtype=np.float32)
        matrices = np.ascontiguousarray(matrices, dtype=np.float32)
        if group_films.ndim != 4 or group_films.shape[3] != 4 or matrices.shape != (group_films.shape[0], 3, 3):
            raise ValueError("group_films [G,H,W,4] and matrices [G,3,3]")
        G, h, w, _ = group_films.shape
        out = np.zeros((h, w, 4), np.float32)
        self.call("light_groups_mix", w, h, G, _fp(group_films), _fp(matrices), _fp(out))
        return out

    def light_groups_relamp_matrix(self, rd, bins, responses, groups, old_curve, new_curve, gain=None, curves=None, curve_data=None, filter=None, subsamples=1):
        """pt_light_groups_relamp_matrix: float32 [K, G, bins], the matrix of a re-lamp of `groups` = G groups rendered with `bins` bins.  responses, curves,
        curve_data, filter and subsamples are spectral_response_matrix's.  old_curve[g] / new_curve[g]: indices into `curves` — group g's emission curve as it
        was rendered and the one to see it under — or RELAMP_KEEP (None); gain [G] (None = all 1).  Entry [k, g, b] integrates response k times
        new / old over bin b.  With KEEP and gain 1 a group's rows are spectral_response_matrix's bit for bit.  Host only."""
        self.entry("light_groups_relamp_matrix")
        responses = [int(r) for r in responses]
        K, G = len(responses), int(groups)
        keep = lambda seq: [RELAMP_KEEP if c is None else int(c) for c in seq]
        old_curve, new_curve = keep(old_curve), keep(new_curve)
        if len(old_curve) != G or len(new_curve) != G:
            raise ValueError("old_curve and new_curve: one entry per group")
        curves = list(curves) if curves is not None else []
        carr = (Curve * max(len(curves), 1))(*curves)
        cd = np.ascontiguousarray(curve_data if curve_data is not None else [], dtype=np.float32).ravel()
        rarr = (C.c_int32 * max(K, 1))(*responses)
        oarr, narr = (C.c_int32 * max(G, 1))(*old_curve), (C.c_int32 * max(G, 1))(*new_curve)
        garr = None
        if gain is not None:
            garr = np.ascontiguousarray(gain, dtype=np.float32).ravel()
            if garr.size != G:
                raise ValueError("gain: one factor per group")
        matrix = np.zeros((K, max(G, 0), max(int(bins), 0)), np.float32)
        sd = SpectralDesc(bins)
        self.call("light_groups_relamp_matrix", C.byref(rd), C.byref(sd), carr if curves else None, len(curves), _fp(cd) if cd.size else None, cd.size, K, rarr,
                  SPECTRAL_NO_FILTER if filter is None else int(filter), subsamples, G, oarr, narr, _fp(garr), _fp(matrix))
        return matrix

    def light_groups_relamp(self, group_spectral, matrix):
        """pt_light_groups_relamp: group_spectral [G,B,H,W] developed by matrix [K,G,B] (light_groups_relamp_matrix makes one): float32 [K,H,W], out[k] = the f32
        fold of matrix[k,g,b] * group_spectral[g,b] over the planes g * B + b ascending."""
        self.entry("light_groups_relamp")
        group_spectral = np.ascontiguousarray(group_spectral, dtype=np.float32)
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if group_spectral.ndim != 4 or matrix.ndim != 3 or matrix.shape[1:] != group_spectral.shape[:2]:
            raise ValueError("group_spectral [G,B,H,W] and matrix [K,G,B]")
        G, bins, h, w = group_spectral.shape
        K = matrix.shape[0]
        out = np.zeros((K, h, w), np.float32)
        self.call("light_groups_relamp", w, h, G, bins, K, _fp(matrix), _fp(group_spectral), _fp(out))
        return out

    def denoise_light_groups(self, film, counts, stats, guides, group_films, albedo=None, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0,
                             device=0, variance=False):
        """pt_denoise_light_groups: the joint filter over the film and its group films [G,H,W,4] — the taps and weights of denoise_film (with `albedo` [H,W,4]:
        of its demodulated form, and the groups are divided by the albedo too) applied to every group channel.  Returns (denoised film, denoised group films[,
        variance]); the group films are bit for bit denoise_spectral_albedo's planes for the 3G planes of the groups' channels."""
        self.entry("denoise_light_groups")
        h, w, film, counts, stats, guides, group_films, albedo, _ = _filter_inputs(film, counts, stats, guides, group_films, _GROUPS_LAYOUT, albedo)
        d = DenoiseDesc(w, h, iterations, sigma_luminance, sigma_depth, normal_power_log2, device)
        out, var, out_groups = _filter_outputs(h, w, variance, group_films)
        self.call("denoise_light_groups", C.byref(d), group_films.shape[0], _fp(film), _u32p(counts), _f64p(stats), _fp(guides), _fp(albedo), _fp(group_films), _fp(out),
                  _fp(var), _fp(out_groups))
        return (out, out_groups, var) if variance else (out, out_groups)


class Scene:
    """Owns a pt_scene handle created from a SceneBuilder (rust-pathtracer_amd.scene)."""

    def __init__(self, library, builder, tuning=None):
        self.library = library
        self.builder = builder
        # a SceneBuilder (scene.py) or a SceneFile (scene_file.py, the C++ TOML front end)
        desc, keep = builder.desc_and_keepalive() if hasattr(builder, "desc_and_keepalive") else builder.desc()
        self._keep = keep
        handle = C.c_void_p()
        if tuning is not None:
            if library._scene_create_tuned is None:
                raise PtError(PT_ERR_UNSUPPORTED, "this library does not export %sscene_create_tuned (pt_tuning is the HIP engine's)" % library.prefix)
            library.call("scene_create_tuned", C.byref(desc), C.byref(tuning), C.byref(handle))
        else:
            library.call("scene_create", C.byref(desc), C.byref(handle))
        self.handle = handle

    def close(self):
        if self.handle:
            self.library._scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def uses_leaf_sweep(self):
        """True when closest-hit queries on this scene take the leaf sweep (<= 64 leaves) instead of the BVH walk."""
        return bool(self.library._debug_scene_info(self.handle, 4))

    def _call(self, name, *args):
        """Library.call of an entry that takes the scene first."""
        self.library.call(name, self.handle, *args)

    def _render_call(self, name, rd, adaptive=None, groups=None, bins=None, device_mask=None, stats=False, read_groups=True, read_bins=True, passes=False, exprs=None):
        """The one render call behind the render* methods: the entry `name` with the arguments it takes, in the order all of them share — rd,
        adaptive desc, groups desc, spectral desc, device mask, film, counts, stats, group films, spectral, group spectral, profile — and the outputs in
        that order, the stats only with `stats`.  adaptive: (max_samples, step, rel_error, abs_error); groups: (instance_group, environment_group, G or None:
        the largest id, the environment's included, plus one); passes: a path passes desc where the groups desc would stand, and the PATH_PASSES pass films where the
        group films would; exprs: (program, instance_group or None) — the program, the group ids and their number where the groups desc would stand, and the
        program's `outputs` expression films where the group films would; what read_groups / read_bins do not ask for is passed, and returned, as None."""
        self.library.entry(name)
        h, w = rd.height, rd.width
        descs, pointers, outs, prof, table = [rd], [], [], Profile(), []

        def out(*shape, read=True):
            a = np.zeros(shape, dtype=np.float32) if read else None
            pointers.append(_fp(a))
            outs.append(a)
        out(h, w, 4)
        if adaptive is not None:
            descs.append(AdaptiveDesc(*adaptive))
            counts = np.zeros((h, w), dtype=np.uint32)
            st = np.zeros((h, w, 2), dtype=np.float64) if stats else None
            pointers += [_u32p(counts), _f64p(st)]
            outs += [counts, st] if stats else [counts]
        if groups is not None:
            instance_group, environment_group, G = groups
            ids = np.ascontiguousarray(instance_group, dtype=np.uint8).reshape(-1)
            G = int(G) if G is not None else int(max([int(environment_group)] + [int(i) for i in ids])) + 1
            descs.append(LightGroupsDesc(G, ids.size, _u8p(ids), int(environment_group)))
            out(max(G, 0), h, w, 4, read=read_groups)
        if passes:
            descs.append(PathPassesDesc())
            out(PATH_PASSES, h, w, 4, read=read_groups)
        if exprs is not None:
            program, instance_group = exprs
            ids = None if instance_group is None else np.ascontiguousarray(instance_group, dtype=np.uint8).reshape(-1)
            descs.append(program)
            table = [_u8p(ids), 0 if ids is None else ids.size]
            out(min(max(int(program.outputs), 0), PATH_EXPRS_MAX), h, w, 4, read=read_groups)
        if bins is not None:
            descs.append(SpectralDesc(bins))
            out(max(int(bins), 0), h, w, read=read_bins)
            if groups is not None:
                out(max(G, 0), max(int(bins), 0), h, w, read=read_bins)
        mask = [] if device_mask is None else [C.c_uint64(device_mask)]
        self._call(name, *[C.byref(d) for d in descs], *table, *mask, *pointers, C.byref(prof))
        return (*outs, prof)

    def render(self, rd):
        return self._render_call("render", rd)

    def render_multi(self, rd, device_mask=0):
        """pt_render_multi: every device of the mask (0 = all) from one blocking call."""
        return self._render_call("render_multi", rd, device_mask=device_mask)

    def render_spectral(self, rd, bins):
        """pt_render_spectral: (film, spectral, profile) — film [H,W,4] is render(rd)'s bit for bit; spectral [bins,H,W] f32 holds per pixel the mean
        per-sample energy that fell into each of `bins` equal wavelength bins over rd's bounds (Library.spectral_bin_centres gives their centres)."""
        return self._render_call("render_spectral", rd, bins=bins)

    def render_spectral_multi(self, rd, bins, device_mask=0):
        """pt_render_spectral_multi: render_spectral on every device of the mask (0 = all) from one blocking call, its outputs bit for bit.  Every device hands
        over the bins of its own tiles; they stay on it as its part of the scene's resident film."""
        return self._render_call("render_spectral_multi", rd, bins=bins, device_mask=device_mask)

    def render_adaptive(self, rd, max_samples, rel_error, abs_error=0.0, step=0, stats=False):
        """pt_render_adaptive: rd.spp samples per pixel at least, max_samples at most, `step` more per round (0 = rd.spp) while a pixel or one of its
        neighbours has not reached the target error.  Returns (film, counts[, stats], profile): counts [H,W] u32, stats [H,W,2] f64 (S1, S2)."""
        return self._render_call("render_adaptive", rd, (max_samples, step, rel_error, abs_error), stats=stats)

    def render_adaptive_multi(self, rd, max_samples, rel_error, abs_error=0.0, step=0, stats=False, device_mask=0):
        """pt_render_adaptive_multi: render_adaptive on every device of the mask (0 = all) from one blocking call, its outputs bit for bit.
        Returns (film, counts[, stats], profile) as render_adaptive does."""
        return self._render_call("render_adaptive_multi", rd, (max_samples, step, rel_error, abs_error), device_mask=device_mask, stats=stats)

    def render_adaptive_spectral(self, rd, bins, max_samples, rel_error, abs_error=0.0, step=0, stats=False):
        """pt_render_adaptive_spectral: render_adaptive with a spectral film.  Returns (film, counts[, stats], spectral, profile): film, counts and stats are
        render_adaptive's bit for bit; spectral [bins,H,W] holds per pixel the bins of render_spectral at that pixel's own sample count."""
        return self._render_call("render_adaptive_spectral", rd, (max_samples, step, rel_error, abs_error), bins=bins, stats=stats)

    def render_adaptive_spectral_multi(self, rd, bins, max_samples, rel_error, abs_error=0.0, step=0, stats=False, device_mask=0):
        """pt_render_adaptive_spectral_multi: render_adaptive_spectral on every device of the mask (0 = all) from one blocking call, its outputs bit for bit.
        Returns (film, counts[, stats], spectral, profile) as render_adaptive_spectral does."""
        return self._render_call("render_adaptive_spectral_multi", rd, (max_samples, step, rel_error, abs_error), bins=bins, device_mask=device_mask, stats=stats)

    def render_light_groups(self, rd, instance_group, environment_group=0, groups=None, read_groups=True):
        """pt_render_light_groups: (film, group_films, profile) — film [H,W,4] is render(rd)'s bit for bit; group_films [G,H,W,4] holds per group the film of the
        energy its emitters contributed.  instance_group: one group id per instance of the scene; groups: G (None = the largest id + 1); read_groups False leaves
        the group films on the device alone (group_films is None) for light_groups_mix_resident."""
        return self._render_call("render_light_groups", rd, groups=(instance_group, environment_group, groups), read_groups=read_groups)

    def render_light_groups_multi(self, rd, instance_group, environment_group=0, groups=None, read_groups=True, device_mask=0):
        """pt_render_light_groups_multi: render_light_groups on every device of the mask (0 = all) from one blocking call, its outputs bit for bit.  Every device
        hands over the group films of its own tiles (read_groups False: none of them) and keeps them, packed, as its part of the scene's resident group films."""
        return self._render_call("render_light_groups_multi", rd, groups=(instance_group, environment_group, groups), device_mask=device_mask, read_groups=read_groups)

    def render_light_groups_spectral(self, rd, bins, instance_group, environment_group=0, groups=None, read_groups=True, read_bins=True):
        """pt_render_light_groups_spectral: (film, group_films, spectral, group_spectral, profile) — film [H,W,4] and group_films [G,H,W,4] are
        render_light_groups' bit for bit, spectral [bins,H,W] is render_spectral's bit for bit, and group_spectral [G,bins,H,W] holds per group the bins of the
        energy its emitters contributed.  read_groups False leaves the group films on the device alone (None), read_bins False the total and the group bins (both
        None), for light_groups_relamp_resident and spectral_project_resident."""
        return self._render_call("render_light_groups_spectral", rd, groups=(instance_group, environment_group, groups), bins=bins, read_groups=read_groups,
                                 read_bins=read_bins)

    def render_adaptive_light_groups(self, rd, max_samples, rel_error, instance_group, environment_group=0, groups=None, abs_error=0.0, step=0, stats=False, read_groups=True):
        """pt_render_adaptive_light_groups: (film, counts[, stats], group_films, profile) — film, counts and stats are render_adaptive's bit for bit; group_films
        [G,H,W,4] holds per pixel the group films of render_light_groups at that pixel's own sample count.  The scene then holds the resident film of
        render_adaptive and the group films of render_light_groups, paired for denoise_light_groups_resident.  read_groups False: group_films is None."""
        return self._render_call("render_adaptive_light_groups", rd, (max_samples, step, rel_error, abs_error), (instance_group, environment_group, groups), stats=stats,
                                 read_groups=read_groups)

    def render_adaptive_light_groups_multi(self, rd, max_samples, rel_error, instance_group, environment_group=0, groups=None, abs_error=0.0, step=0, stats=False,
                                           read_groups=True, device_mask=0):
        """pt_render_adaptive_light_groups_multi: render_adaptive_light_groups on every device of the mask (0 = all) from one blocking call, its outputs bit for
        bit.  Over more than one (virtual) device the group films stay resident as packed shards, paired with no film, until resident_assemble (after a call
        with stats=True) gathers film and group films on the scene's device."""
        return self._render_call("render_adaptive_light_groups_multi", rd, (max_samples, step, rel_error, abs_error), (instance_group, environment_group, groups),
                                 device_mask=device_mask, stats=stats, read_groups=read_groups)

    def render_path_passes(self, rd, read_passes=True):
        """pt_render_path_passes: (film, pass_films, profile) — film [H,W,4] is render(rd)'s bit for bit; pass_films [8,H,W,4] holds, in the order of
        PATH_PASS_NAMES, the film of the energy that travelled each way.  The pass films stay on the device as the scene's resident group films (8 groups):
        light_groups_resident and light_groups_mix_resident follow.  read_passes False leaves them there alone (pass_films is None)."""
        return self._render_call("render_path_passes", rd, passes=True, read_groups=read_passes)

    def render_adaptive_path_passes(self, rd, max_samples, rel_error, abs_error=0.0, step=0, stats=False, read_passes=True):
        """pt_render_adaptive_path_passes: (film, counts[, stats], pass_films, profile) — film, counts and stats are render_adaptive's bit for bit; pass_films
        [8,H,W,4] holds per pixel the pass films of render_path_passes at that pixel's own sample count.  The scene then holds the resident film and the pass
        films as its group films, paired for denoise_light_groups_resident.  read_passes False: pass_films is None."""
        return self._render_call("render_adaptive_path_passes", rd, (max_samples, step, rel_error, abs_error), stats=stats, passes=True, read_groups=read_passes)

    def _expr_program(self, exprs, environment_group):
        """exprs as a render takes them: a PathExprProgram as it is, else text(s) for Library.path_expr_compile."""
        return exprs if isinstance(exprs, PathExprProgram) else self.library.path_expr_compile(exprs, environment_group)

    def render_path_exprs(self, rd, exprs, instance_group=None, environment_group=0, read_films=True):
        """pt_render_path_exprs: (film, expr_films, profile) — film [H,W,4] is render(rd)'s bit for bit; expr_films [K,H,W,4] holds per expression the film of the
        energy of exactly the paths it matches.  exprs: path expressions (a text, a sequence of up to PATH_EXPRS_MAX, or a compiled PathExprProgram, whose own
        environment group then holds); instance_group: one light group id below 8 per instance of the scene for L0..L7 (None: every instance in group 0);
        environment_group: the group E0..E7 finds the environment in.  The films stay on the device as the scene's resident group films (K groups), as pass films
        do.  read_films False leaves them there alone (expr_films is None)."""
        return self._render_call("render_path_exprs", rd, exprs=(self._expr_program(exprs, environment_group), instance_group), read_groups=read_films)

    def render_adaptive_path_exprs(self, rd, max_samples, rel_error, exprs, instance_group=None, environment_group=0, abs_error=0.0, step=0, stats=False, read_films=True):
        """pt_render_adaptive_path_exprs: (film, counts[, stats], expr_films, profile) — film, counts and stats are render_adaptive's bit for bit; expr_films
        [K,H,W,4] holds per pixel the films of render_path_exprs at that pixel's own sample count.  The scene then holds the resident film and the expression
        films as its group films, paired for denoise_light_groups_resident.  read_films False: expr_films is None."""
        return self._render_call("render_adaptive_path_exprs", rd, (max_samples, step, rel_error, abs_error), stats=stats,
                                 exprs=(self._expr_program(exprs, environment_group), instance_group), read_groups=read_films)

    def _resident_dims(self, name, count=3):
        """A pt_*_resident query: (width, height, planes[, bins]) of what a render left on the device(s), None when it left none."""
        dims = [C.c_uint32() for _ in range(count)]
        self._call(name, *[C.byref(d) for d in dims])
        return tuple(d.value for d in dims) if dims[2].value else None

    def spectral_resident(self):
        """pt_spectral_resident: (width, height, bins) of the spectral film the last successful spectral render (one device or a node) left on the device(s), or
        None when the scene holds none."""
        return self._resident_dims("spectral_resident")

    def light_groups_resident(self):
        """pt_light_groups_resident: (width, height, groups) of the group films the last successful light-group render left on the device(s), or None."""
        return self._resident_dims("light_groups_resident")

    def light_groups_spectral_resident(self):
        """pt_light_groups_spectral_resident: (width, height, groups, bins) of the group bins the last successful render_light_groups_spectral left on the device, or
        None (any other group render ends them)."""
        return self._resident_dims("light_groups_spectral_resident", 4)

    def light_groups_denoised_resident(self):
        """pt_light_groups_denoised_resident: (width, height, groups) of the denoised group films denoise_light_groups_resident left on the device, or None."""
        return self._resident_dims("light_groups_denoised_resident")

    def light_groups_relamp_resident(self, matrix):
        """pt_light_groups_relamp_resident: Library.light_groups_relamp of the resident group bins with matrix [K,G,B] — float32 [K,H,W], bit for bit what the
        host-array entry gives for the bins render_light_groups_spectral returned; only the matrix goes up and K planes come back."""
        self.library.entry("light_groups_relamp_resident")
        res = self.light_groups_spectral_resident()
        if res is None:
            w = h = G = B = 0
        else:
            w, h, G, B = res
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if res is not None and (matrix.ndim != 3 or matrix.shape[1:] != (G, B)):
            raise ValueError("matrix [K,%d,%d] for the resident group bins" % (G, B))
        K = matrix.shape[0] if matrix.ndim else 0
        out = np.zeros((K, h, w), np.float32)
        self._call("light_groups_relamp_resident", K, _fp(matrix), _fp(out) if out.size else _fp(np.zeros(1, np.float32)))
        return out

    def denoise_light_groups_resident(self, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, film=True, variance=False, groups=True):
        """pt_denoise_light_groups_resident: Library.denoise_light_groups over the resident film, guides (and albedo, which selects demodulation) and the group
        films render_adaptive_light_groups left with that film.  Returns the tuple of what was asked for, in this order: the denoised film [H,W,4] (film), its
        variance [H,W] (variance), the denoised group films [G,H,W,4] (groups) — one array when one is asked for, None when none is.  What is not asked for
        does not cross the bus; the denoised group films stay on the device for light_groups_mix_resident(m, denoised=True)."""
        self.library.entry("denoise_light_groups_resident")
        w, h, _, _ = self.resident_info()
        res = self.light_groups_resident()
        G = res[2] if res else 0
        d = ResidentDenoiseDesc(DenoiseDesc(0, 0, iterations, sigma_luminance, sigma_depth, normal_power_log2, 0), 0)
        out = np.zeros((h, w, 4), np.float32) if film else None
        var = np.zeros((h, w), np.float32) if variance else None
        gf = np.zeros((G, h, w, 4), np.float32) if groups else None
        self._call("denoise_light_groups_resident", C.byref(d), _fp(out), _fp(var), _fp(gf))
        return _asked(out, var, gf)

    def _host_guides(self, rd, guide_samples, specular_chain, albedo):
        """(guides, albedo or None) on the host for a filter over host arrays: at the end of the specular chains when specular_chain is not None, else with
        the albedo of the first hit, else the plain guides."""
        if specular_chain is not None:
            return self.render_guides_chain(rd, guide_samples, specular_chain, albedo=albedo)
        if albedo:
            return self.render_guides_albedo(rd, guide_samples)
        return self.render_guides(rd, guide_samples), None

    def render_denoised_light_groups(self, rd, instance_group, environment_group=0, groups=None, max_samples=None, rel_error=0.0, abs_error=0.0, step=0, guide_samples=4,
                                     specular_chain=0, albedo=False, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, device_mask=None,
                                     assemble=False):
        """render_adaptive_light_groups with statistics (max_samples None = rd.spp: a fixed count), resident_guides (with `albedo`: the albedo too, and the filter
        demodulates by it; `specular_chain` > 0: guides at the end of every sample's specular chain) and denoise_light_groups_resident, in one call:
        (film, denoised, group_films, denoised_group_films, counts, profile).  The denoised group films stay on the device for the relight.  A device_mask
        routes the render through render_adaptive_light_groups_multi; guides and the joint filter then run over host arrays on the first device of the mask
        (render_guides*, Library.denoise_light_groups), and the denoised group films are on the host alone.  `assemble` (with a device_mask only): the node
        render's film and packed group films are assembled on the scene's device (resident_assemble) and guides and filter run resident, as without a mask."""
        mx = rd.spp if max_samples is None else max_samples
        if assemble and device_mask is None:
            raise ValueError("assemble gathers a node render: it needs a device_mask")
        if device_mask is None:
            film, counts, st, group_films, prof = self.render_adaptive_light_groups(rd, mx, rel_error, instance_group, environment_group, groups, abs_error, step, stats=True)
        else:
            film, counts, st, group_films, prof = self.render_adaptive_light_groups_multi(rd, mx, rel_error, instance_group, environment_group, groups, abs_error, step,
                                                                                          stats=True, device_mask=device_mask)
        if assemble:
            self._assemble_node_render()
        elif device_mask is not None and not (self.resident_info()[3] & RESIDENT_FILM):   # (a mask that came down to the scene's device left the film resident itself)
            guides, alb = self._host_guides(rd, guide_samples, specular_chain if specular_chain > 0 else None, albedo)
            den, den_groups = self.library.denoise_light_groups(film, counts, st, guides, group_films, albedo=alb, iterations=iterations,
                                                                sigma_luminance=sigma_luminance, sigma_depth=sigma_depth, normal_power_log2=normal_power_log2,
                                                                device=_first_device(device_mask))[:2]
            return film, den, group_films, den_groups, counts, prof
        self.resident_guides(rd, guide_samples, specular_chain, albedo=albedo)
        den, den_groups = self.denoise_light_groups_resident(iterations, sigma_luminance, sigma_depth, normal_power_log2)
        return film, den, group_films, den_groups, counts, prof

    def light_groups_mix_resident(self, matrices, denoised=False):
        """pt_light_groups_mix_resident: Library.light_groups_mix of the resident group films with matrices [G,3,3] — float32 [H,W,4], bit for bit what the host-array
        entry gives for the films render_light_groups returned; only the matrices go up and one film comes back.  `denoised`:
        pt_light_groups_mix_resident_denoised, the same of the group films that denoise_light_groups_resident left on the device."""
        name = "light_groups_mix_resident_denoised" if denoised else "light_groups_mix_resident"
        self.library.entry(name)
        res = self.light_groups_denoised_resident() if denoised else self.light_groups_resident()
        if res is None:
            raise PtError(PT_ERR_INVALID_ARGUMENT, "the scene has no resident denoised group films" if denoised else "the scene has no resident group films")
        matrices = np.ascontiguousarray(matrices, dtype=np.float32)
        if matrices.shape != (res[2], 3, 3):
            raise ValueError("matrices [G,3,3] with G = %d" % res[2])
        out = np.zeros((res[1], res[0], 4), np.float32)
        self._call(name, _fp(matrices), _fp(out))
        return out

    def resident_info(self):
        """pt_resident_info: (width, height, bins, parts) of the scene's resident set — parts a set of RESIDENT_* bits, all zeros when nothing is resident."""
        info = ResidentInfo()
        self._call("resident_info", C.byref(info))
        return info.width, info.height, info.bins, info.parts

    def resident_guides(self, rd, guide_samples=4, specular_chain=0, alpha_max=0.0, albedo=False, bin_albedo=False):
        """pt_resident_guides: render_guides (render_guides_albedo with albedo, render_guides_bin_albedo over the resident bins with bin_albedo too; with
        specular_chain > 0 at the end of every sample's specular chain) for the resident film, the outputs kept on the device as resident parts."""
        cd = GuideChainDesc(specular_chain, alpha_max)
        flags = (RESIDENT_ALBEDO if albedo else 0) | (RESIDENT_BIN_ALBEDO if bin_albedo else 0)
        self._call("resident_guides", C.byref(rd), guide_samples, C.byref(cd) if specular_chain > 0 else None, flags)

    def resident_load(self, film=None, counts=None, stats=None, guides=None, spectral=None, albedo=None, bin_albedo=None):
        """pt_resident_load: host arrays adopted as resident parts — film [H,W,4], counts [H,W] u32 and stats [H,W,2] f64 together, guides [H,W,4],
        spectral [B,H,W], albedo [H,W,4], bin_albedo [B,H,W]; what is None stays as it is.  The size is taken from the arrays given."""
        def arr(a, dtype):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype)
        film, counts, stats = arr(film, np.float32), arr(counts, np.uint32), arr(stats, np.float64)
        spectral, guides, albedo, bin_albedo = (arr(a, np.float32) for a in (spectral, guides, albedo, bin_albedo))
        sizes = {a.shape[:2] for a in (film, counts, stats, guides, albedo) if a is not None} | {a.shape[1:] for a in (spectral, bin_albedo) if a is not None}
        nbins = {a.shape[0] for a in (spectral, bin_albedo) if a is not None}
        if len(sizes) > 1 or len(nbins) > 1 or any(a is not None and a.ndim != 3 for a in (film, stats, spectral, guides, albedo, bin_albedo)):
            raise ValueError("film [H,W,4], counts [H,W], stats [H,W,2], spectral [B,H,W], guides [H,W,4], albedo [H,W,4] and bin_albedo [B,H,W] of one size")
        h, w = sizes.pop() if sizes else (0, 0)
        for a, last in ((film, 4), (stats, 2), (guides, 4), (albedo, 4)):
            if a is not None and a.shape[2] != last:
                raise ValueError("film, guides and albedo [H,W,4], stats [H,W,2]")
        self._call("resident_load", w, h, nbins.pop() if nbins else 0, _fp(film), _u32p(counts), _f64p(stats), _fp(spectral), _fp(guides), _fp(albedo), _fp(bin_albedo))

    def resident_assemble(self, staged=False):
        """pt_resident_assemble: the pieces the last adaptive node render (render_adaptive_multi, render_adaptive_spectral_multi with stats=True) left on the
        devices gathered on the scene's own device as the resident film (and bins), device to device: resident_guides and denoise_resident then follow as after
        a one-device render.  `staged`: every shard of the bins goes through the staging copy, also one that lies on the scene's device; the bits are the same."""
        self._call("resident_assemble", RESIDENT_ASSEMBLE_STAGED if staged else 0)

    def resident_read(self, film=True, counts=True, stats=True, spectral=False):
        """pt_resident_read: the resident film [H,W,4] (film), counts [H,W] u32 (counts), stats [H,W,2] f64 (stats) and bins [B,H,W] (spectral) copied to the
        host, however they became resident.  Returns the tuple of what was asked for, in this order — one array when one is asked for, None when none is."""
        w, h, bins, _ = self.resident_info()
        f = np.zeros((h, w, 4), np.float32) if film else None
        c = np.zeros((h, w), np.uint32) if counts else None
        st = np.zeros((h, w, 2), np.float64) if stats else None
        sp = np.zeros((bins, h, w), np.float32) if spectral else None
        self._call("resident_read", _fp(f), _u32p(c), _f64p(st), _fp(sp))
        return _asked(f, c, st, sp)

    def _assemble_node_render(self):
        """Behind a node render: the film resident on the scene's device — it already is when the mask came down to this one device."""
        if not (self.resident_info()[3] & RESIDENT_FILM):
            self.resident_assemble()

    def denoise_resident(self, iterations=0, sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, film=True, variance=False, spectral=False, planar=False):
        """pt_denoise_resident: the filter over the resident set, where it lies.  Returns the tuple of what was asked for, in this order: the denoised film
        [H,W,4] (film), its variance [H,W] (variance), the denoised bins [B,H,W] (spectral) — one array when one is asked for, None when none is.  What is
        not asked for does not cross the bus; all of it stays resident.  `planar`: the passes over plane-major bins; the bits are the same."""
        w, h, bins, _ = self.resident_info()
        d = ResidentDenoiseDesc(DenoiseDesc(0, 0, iterations, sigma_luminance, sigma_depth, normal_power_log2, 0), RESIDENT_PLANAR_GATHER if planar else 0)
        out = np.zeros((h, w, 4), np.float32) if film else None
        var = np.zeros((h, w), np.float32) if variance else None
        sp = np.zeros((bins, h, w), np.float32) if spectral else None
        self._call("denoise_resident", C.byref(d), _fp(out), _fp(var), _fp(sp))
        return _asked(out, var, sp)

    def spectral_project_resident(self, matrix, denoised=False):
        """pt_spectral_project_resident: Library.spectral_project of the resident spectral film with matrix [K,B] — float32 [K,H,W], bit for bit what
        spectral_project gives for the array that render returned — without the bins crossing the bus.  `denoised`:
        pt_spectral_project_resident_denoised, the same of the bins that denoise_resident left on the device."""
        name = "spectral_project_resident_denoised" if denoised else "spectral_project_resident"
        self.library.entry(name)
        matrix = np.ascontiguousarray(matrix, dtype=np.float32)
        if matrix.ndim != 2:
            raise ValueError("matrix [K,B]")
        if denoised:
            w, h, bins, parts = self.resident_info()
            known = parts & RESIDENT_DENOISED_BINS
        else:
            res = self.spectral_resident()
            w, h, bins = res if res else (0, 0, matrix.shape[1])   # (no resident film: the entry refuses, with its message)
            known = True
        if known and matrix.shape[1] != bins:
            raise ValueError("matrix [K,B] with B = %d, the resident film's bins" % bins)
        out = np.zeros((matrix.shape[0], h, w), np.float32)
        self._call(name, matrix.shape[0], _fp(matrix), _fp(out))
        return out

    def render_guides(self, rd, samples=4):
        """pt_render_guides: [H,W,4] f32 = the mean first-hit normal and distance over camera samples 0 .. samples-1 of the render `rd`."""
        self.library.entry("render_guides")
        g = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        self._call("render_guides", C.byref(rd), samples, _fp(g))
        return g

    def render_guides_albedo(self, rd, samples=4):
        """pt_render_guides_albedo: (guides, albedo), [H,W,4] f32 each — render_guides' output and, from the same probes, the mean first-hit albedo as XYZ
        factors (W = 0)."""
        self.library.entry("render_guides_albedo")
        g = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        a = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        self._call("render_guides_albedo", C.byref(rd), samples, _fp(g), _fp(a))
        return g, a

    def render_guides_chain(self, rd, guide_samples=4, max_chain=8, alpha_max=0.0, albedo=True):
        """pt_render_guides_chain: (guides, albedo), [H,W,4] f32 each, taken at the end of every sample's specular chain — through passthrough boundaries and
        GGX materials with alpha <= alpha_max (0 = 0.01), at most max_chain vertices (0 = render_guides_albedo).  albedo=False: (guides, None)."""
        self.library.entry("render_guides_chain")
        g = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        a = np.zeros((rd.height, rd.width, 4), dtype=np.float32) if albedo else None
        cd = GuideChainDesc(max_chain, alpha_max)
        self._call("render_guides_chain", C.byref(rd), guide_samples, C.byref(cd), _fp(g), _fp(a))
        return g, a

    def render_mattes(self, rd, samples, key="instance", ranks=6, read=True):
        """pt_render_mattes: (keys [R,H,W] u32, coverage [R,H,W] f32, overflow [H,W] u32) — per pixel the `ranks` keys that most of the camera samples
        0 .. samples-1 of the render `rd` saw ("instance": pt_hit.instance, "material": the packed MaterialId; MATTE_SKY for a miss, MATTE_NONE for an empty
        rank) with their share of the samples, and the samples that found no free rank.  read=False: nothing is copied back (None); the ranks stay on the
        device for matte_extract_resident either way."""
        self.library.entry("render_mattes")
        md = MatteDesc(samples, ranks, MATTE_KEYS[key] if key in MATTE_KEYS else key)
        planes = (max(int(ranks), 0), rd.height, rd.width)
        keys = np.zeros(planes, np.uint32) if read else None
        coverage = np.zeros(planes, np.float32) if read else None
        overflow = np.zeros((rd.height, rd.width), np.uint32) if read else None
        self._call("render_mattes", C.byref(rd), C.byref(md), _u32p(keys), _fp(coverage), _u32p(overflow))
        return (keys, coverage, overflow) if read else None

    def mattes_resident(self):
        """pt_mattes_resident: (width, height, ranks, samples) of the matte the last successful render_mattes left on the device; refused before one."""
        dims = [C.c_uint32() for _ in range(4)]
        self._call("mattes_resident", *[C.byref(d) for d in dims])
        return tuple(d.value for d in dims)

    def matte_extract_resident(self, selections):
        """pt_matte_extract_resident: Library.matte_extract of the resident matte — float32 [M,H,W], bit for bit what the host-array entry gives for the ranks
        render_mattes returned; only the selections go up and M planes come back."""
        self.library.entry("matte_extract_resident")
        w, h, _, _ = self.mattes_resident()
        M, offsets, selected = matte_selections(selections)
        out = np.zeros((M, h, w), np.float32)
        self._call("matte_extract_resident", M, _u32p(offsets), _u32p(selected), _fp(out))
        return out

    def render_guides_bin_albedo(self, rd, bins, guide_samples=4, max_chain=0, alpha_max=0.0):
        """pt_render_guides_bin_albedo: (guides [H,W,4], albedo [H,W,4], bin_albedo [bins,H,W]) from one set of probes — render_guides_albedo's outputs, or with
        max_chain > 0 render_guides_chain's, and the mean reflectance of the same guide samples at the centre wavelength of each of the render's `bins` bins."""
        self.library.entry("render_guides_bin_albedo")
        g = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        a = np.zeros((rd.height, rd.width, 4), dtype=np.float32)
        ba = np.zeros((max(int(bins), 0), rd.height, rd.width), dtype=np.float32)
        cd = GuideChainDesc(max_chain, alpha_max)
        self._call("render_guides_bin_albedo", C.byref(rd), guide_samples, C.byref(cd) if max_chain > 0 else None, bins, _fp(g), _fp(a), _fp(ba))
        return g, a, ba

    def render_denoised(self, rd, max_samples=None, rel_error=0.0, abs_error=0.0, step=0, guide_samples=4, iterations=0, sigma_luminance=0.0, sigma_depth=0.0,
                        normal_power_log2=0, device_mask=None, albedo=False, specular_chain=None, resident=False, assemble=False):
        """An adaptive render with statistics (max_samples None = rd.spp: a fixed count), its guides, and the filter: (film, denoised, counts, profile).
        `device_mask` (not None) routes the render through render_adaptive_multi; the filter then runs on the first device of the mask.  `albedo`: the
        guides come with the albedo (render_guides_albedo) and the filter demodulates the film by it.  `specular_chain` (not None): the guides, and the
        albedo if asked for, come from render_guides_chain with this max_chain.  `resident`: guides and filter run on what the render left on the device
        (resident_guides, denoise_resident); the tuple is the same, bit for bit.  A node render leaves no such film: refused with a device_mask.
        `assemble` (with a device_mask only): the node render's pieces are assembled on the scene's device (resident_assemble) and guides and filter run
        there, resident; the tuple is the same, bit for bit."""
        mx = rd.spp if max_samples is None else max_samples
        if assemble and device_mask is None:
            raise PtError(PT_ERR_UNSUPPORTED, "render_denoised: assemble=True needs a device_mask (it assembles a node render; resident=True is the one-device form)")
        if resident and device_mask is not None:
            raise PtError(PT_ERR_UNSUPPORTED, "render_denoised: resident=True takes no device_mask (a node render leaves no film one device can filter)")
        if device_mask is None:
            film, counts, st, prof = self.render_adaptive(rd, mx, rel_error, abs_error, step, stats=True)
        else:
            film, counts, st, prof = self.render_adaptive_multi(rd, mx, rel_error, abs_error, step, stats=True, device_mask=device_mask)
        if resident or assemble:
            if assemble:
                self._assemble_node_render()
            self.resident_guides(rd, guide_samples, specular_chain or 0, albedo=albedo)
            return film, self.denoise_resident(iterations, sigma_luminance, sigma_depth, normal_power_log2), counts, prof
        guides, alb = self._host_guides(rd, guide_samples, specular_chain, albedo)
        den = self.library.denoise_film(film, counts, st, guides, iterations, sigma_luminance, sigma_depth, normal_power_log2, _first_device(device_mask or 0), albedo=alb)
        return film, den, counts, prof

    def render_denoised_spectral(self, rd, bins, max_samples=None, rel_error=0.0, guide_samples=4, specular_chain=0, abs_error=0.0, step=0, iterations=0,
                                 sigma_luminance=0.0, sigma_depth=0.0, normal_power_log2=0, albedo=False, bin_albedo=False, resident=False, assemble=False, device_mask=None):
        """render_adaptive_spectral with statistics (max_samples None = rd.spp: a fixed count), its guides — render_guides, or render_guides_chain with max_chain
        `specular_chain` when that is positive — and denoise_spectral: (film, denoised, spectral, denoised_spectral, counts, profile).  `albedo` is refused, as
        denoise_spectral refuses it.  `bin_albedo`: guides, XYZ albedo and per-bin albedo come from one render_guides_bin_albedo call (with `specular_chain` as its
        max_chain) and the filter is denoise_spectral_albedo: the film demodulated by the XYZ albedo, the bins by the per-bin albedo.  `device_mask` (not None)
        routes the render through render_adaptive_spectral_multi; the filter then runs on the first device of the mask.  `resident`: guides and filter run on
        what the render left on the device (resident_guides, denoise_resident); the tuple is the same, bit for bit; refused with a device_mask.  `assemble`
        (with a device_mask only): the node render's film and packed shards are assembled on the scene's device (resident_assemble) and guides and filter run
        there, resident: the bins do not go up again; the tuple is the same, bit for bit."""
        if assemble and device_mask is None:
            raise PtError(PT_ERR_UNSUPPORTED, "render_denoised_spectral: assemble=True needs a device_mask (it assembles a node render; resident=True is the one-device form)")
        if albedo:
            raise PtError(PT_ERR_UNSUPPORTED, "render_denoised_spectral takes no albedo: demodulating the bins needs a per-bin albedo (bin_albedo=True renders one)")
        mx = rd.spp if max_samples is None else max_samples
        if resident and device_mask is not None:
            raise PtError(PT_ERR_UNSUPPORTED, "render_denoised_spectral: resident=True takes no device_mask (a node render leaves no film one device can filter)")
        if device_mask is None:
            film, counts, st, spectral, prof = self.render_adaptive_spectral(rd, bins, mx, rel_error, abs_error, step, stats=True)
        else:
            film, counts, st, spectral, prof = self.render_adaptive_spectral_multi(rd, bins, mx, rel_error, abs_error, step, stats=True, device_mask=device_mask)
        filter_args = (iterations, sigma_luminance, sigma_depth, normal_power_log2)
        if resident or assemble:
            if assemble:
                self._assemble_node_render()
            self.resident_guides(rd, guide_samples, specular_chain, albedo=bin_albedo, bin_albedo=bin_albedo)
            den, den_spectral = self.denoise_resident(*filter_args, spectral=True)
        elif bin_albedo:
            guides, alb, balb = self.render_guides_bin_albedo(rd, bins, guide_samples, specular_chain)
            den, den_spectral = self.library.denoise_spectral_albedo(film, counts, st, guides, spectral, alb, balb, *filter_args, _first_device(device_mask or 0))
        else:
            guides, _ = self._host_guides(rd, guide_samples, specular_chain if specular_chain > 0 else None, False)
            den, den_spectral = self.library.denoise_spectral(film, counts, st, guides, spectral, *filter_args, _first_device(device_mask or 0))
        return film, den, spectral, den_spectral, counts, prof

    def render_device(self, rd, film_ptr, stream_ptr=None):
        prof = Profile()
        self._call("render_device", C.byref(rd), C.c_void_p(film_ptr), C.c_void_p(stream_ptr or 0), C.byref(prof))
        return prof

    def intersect(self, origins, directions):
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        hits = np.zeros(o.shape[0], dtype=HIT_DTYPE)
        self._call("intersect", o.shape[0], _fp(o), _fp(d), hits.ctypes.data_as(C.POINTER(Hit)))
        return hits

    def camera_samples(self, rd, pixel, sample):
        """pt_camera_samples: film jitter + wavelength + Camera::get_ray for (pixel id, sample index) pairs of the render `rd`: (origins, directions, lambda)."""
        pixel = np.ascontiguousarray(pixel, dtype=np.uint32).ravel()
        sample = np.ascontiguousarray(sample, dtype=np.uint32).ravel()
        n = pixel.shape[0]
        o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32); lam = np.zeros(n, np.float32)
        self._call("camera_samples", C.byref(rd), n, _u32p(pixel), _u32p(sample), _fp(o), _fp(d), _fp(lam))
        return o, d, lam

    def bsdf_sample(self, material, lam, wi, s2):
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        wi = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
        s2 = np.ascontiguousarray(s2, dtype=np.float32).reshape(-1, 2)
        n = lam.shape[0]
        f = np.zeros(n, np.float32); wo = np.zeros((n, 3), np.float32); pdf = np.zeros(n, np.float32)
        self._call("bsdf_sample", material, n, _fp(lam), _fp(wi), _fp(s2), _fp(f), _fp(wo), _fp(pdf))
        return f, wo, pdf

    def light_sample(self, entry, origins, s2):
        """Hittable::sample of light-list entry `entry` from the points `origins` (n, 3) with samples `s2` (n, 2): world directions (n, 3) and solid-angle pdfs (n,)."""
        if self.library._light_sample is None:
            raise NotImplementedError("%s has no light_sample entry" % self.library.path)
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        s2 = np.ascontiguousarray(s2, dtype=np.float32).reshape(-1, 2)
        n = o.shape[0]
        d = np.zeros((n, 3), np.float32); pdf = np.zeros(n, np.float32)
        self._call("light_sample", entry, n, _fp(o), _fp(s2), _fp(d), _fp(pdf))
        return d, pdf

    def bsdf_eval(self, material, lam, wi, wo):
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        wi = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
        wo = np.ascontiguousarray(wo, dtype=np.float32).reshape(-1, 3)
        n = lam.shape[0]
        f = np.zeros(n, np.float32); pdf = np.zeros(n, np.float32)
        self._call("bsdf_eval", material, n, _fp(lam), _fp(wi), _fp(wo), _fp(f), _fp(pdf))
        return f, pdf

    def emission(self, material, lam, wi):
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        wi = np.ascontiguousarray(wi, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(lam.shape[0], np.float32)
        self._call("emission", material, lam.shape[0], _fp(lam), _fp(wi), _fp(out))
        return out

    def curve_eval(self, curve, lam):
        lam = np.ascontiguousarray(lam, dtype=np.float32)
        out = np.zeros(lam.shape[0], np.float32)
        self._call("curve_eval", curve, lam.shape[0], _fp(lam), _fp(out))
        return out

