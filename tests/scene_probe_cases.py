"""Scenes and records of the device scene probe (HipRenderer.scene_eval / oracle.scene_eval): deterministic, no GPU.

The scene-bound device functions -- tex_fetch, env_ptn_pdf, light_li / light_bound / light_sample_li,
create_bsdf, dg_lookup / dg_lookup2, medium_sample_ray / maj_next -- depart from the reference's shape
(host-side light constants, restated environment tables searched through guide tables, a feature mask that
drops code, densities in kernel arguments, a late crossing distance), and renders hand them only what a few
scenes produce from continuous distributions.  The scenes here are written at run time (nothing large is
committed); each record set is designed for one class of trouble and then filled from a seed.
tests/test_scene_probe_cases.py shows on the CPU, with the oracle alone, that the classes are populated.

Scenes:
    lights       disk and ring lights under identity, rotation + translation, non-uniform scale and shear, radii
                 1e-3 / 1 / 1e3, ring inner ratios 1e-3 / 0.5 / 0.999, a disk with a textured Le, one textured and
                 one constant environment light
    env_*        one textured environment light each: the smooth sky, 37x19 with zero rows at the top, in the
                 middle and at the bottom, a row with a single non-zero texel, a row of equal texels, 1x1, 64x1,
                 1x64 and 65537x1 (the unguided search)
    materials    every material kind with constant and with textured parameters, a roughness texture around the
                 glossy / specular thresholds, a normal map with texels that decode to 0, -z and the tangent
    mat_diffuse, mat_glass, mat_envtex   variants that fit the three narrow builds of the path kernels
    med_*        the media: 2x2x2 / 2x2x3 / 4x3x5 / 255x2x2 grids in boxes with three, two and no power-of-two
                 sides and with sides of 2^-20 and 2^20
"""
import json
import os

import numpy as np

import nart_amd
from nart_amd import scenes

f32 = np.float32
SEED = 20241021
N_FILL = 6000  # seeded records per op and scene, on top of the designed ones (some 10^4 per op and scene)
SENTINEL = f32(-7.5)  # a preset pdf no function produces: shows where a function left its output alone
INF = f32(np.inf)
ONE_BELOW = np.nextafter(f32(1), f32(0))

ENV_TEXTURES = ("sky", "zero_rows", "one_texel_row", "equal_row", "1x1", "64x1", "1x64", "65537x1")
MEDIA = {  # name: (grid (rz, ry, rx), bounds_min, bounds_max)
    "med_222_pow2": ((2, 2, 2), (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)),
    "med_223_two": ((3, 2, 2), (-1.0, -0.25, -0.1), (1.0, 0.25, 0.2)),
    "med_435_none": ((5, 3, 4), (-1.0, -0.8, -0.6), (1.2, 0.9, 1.0)),
    "med_255_tiny": ((2, 2, 255), (0.0, 0.0, 0.0), (2.0 ** -20, 2.0 ** -20, 2.0 ** -20)),
    "med_222_huge": ((2, 2, 2), (-2.0 ** 19, -2.0 ** 19, -2.0 ** 19), (2.0 ** 19, 2.0 ** 19, 2.0 ** 19)),
}
SCENES = ("lights",) + tuple("env_" + t for t in ENV_TEXTURES) + ("materials", "mat_diffuse", "mat_glass", "mat_envtex") + tuple(MEDIA)
OPS = tuple(nart_amd.SCENE_OPS)


def edges(x):
    """x and the nearest float32 on either side."""
    x = f32(x)
    return np.array([np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))], f32)


def u32(a):
    return np.asarray(a, np.uint32).view(f32)


def records(n):
    return np.zeros((n, nart_amd.SCENE_IN_WORDS), f32)


# ------------------------------------------------------------------------------------------------ scenes
def _tri_geo(path):
    """One triangle with UVs: a mesh to carry a material."""
    scenes.write_geo(path, [[0, 1, 2]], [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0.0, 0.0, 1.0)], [[0, 0, 0]],
                     [(0, 0), (1, 0), (0, 1)], [[0, 1, 2]])
    return path


def _rgba(rgb):
    rgb = np.asarray(rgb, f32)
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), f32)], -1)


def env_texture(kind):
    """(H, W, 4) float32 of an environment map; every value is exact in half precision or rounded by the writer."""
    rng = np.random.default_rng([SEED, ENV_TEXTURES.index(kind)])
    if kind == "sky":
        return scenes.sky_texture(32, 16)
    if kind == "zero_rows":
        # Zero rows at the top, in the middle and at the bottom.  A sample reaches a zero row only past the
        # marginal CDF's last step (the search returns the last row whose CDF entry is <= sample.y, and a zero
        # row shares its entry with the row after it), so the texels (exact halves) are drawn again until that
        # step lies a few floats below 1, where samples exist.
        for _ in range(64):
            t = rng.uniform(0.1, 2.0, (19, 37, 3)).astype(np.float16).astype(f32)
            t[[0, 1, 8, 9, 17, 18]] = 0.0
            if env_tables(t)[1][-1] <= np.nextafter(np.nextafter(ONE_BELOW, f32(0)), f32(0)):
                return _rgba(t)
        raise AssertionError("no zero_rows texture whose last CDF step lies below 1")
    if kind == "one_texel_row":
        t = rng.uniform(0.1, 2.0, (9, 12, 3)).astype(f32)
        t[4] = 0.0
        t[4, 7] = (8.0, 4.0, 2.0)
        return _rgba(t)
    if kind == "equal_row":
        t = rng.uniform(0.1, 2.0, (9, 12, 3)).astype(f32)
        t[3] = 0.5
        return _rgba(t)
    h, w = {"1x1": (1, 1), "64x1": (1, 64), "1x64": (64, 1), "65537x1": (1, 65537)}[kind]
    return _rgba(rng.uniform(0.1, 2.0, (h, w, 3)).astype(f32))


ROUGH_W, ROUGH_H = 8, 4


def rough_texture():
    """8x4 roughness texels t (alpha = t^2): rows around the t whose square is 1e-4 and 1e-3 (halves 16 apart
    either way), a row of 0 / 1 / 0.5 and a row of ordinary values."""
    t = np.zeros((ROUGH_H, ROUGH_W), f32)
    for row, thr in ((0, 1e-4), (1, 1e-3)):
        c = np.float16(np.sqrt(thr)).view(np.uint16)
        t[row] = (np.uint16(c) + np.arange(-4, 4, dtype=np.int16).astype(np.uint16) * np.uint16(4)).astype(np.uint16).view(np.float16)
    t[2] = [0, 1, 0.5, 0, 1, 0.5, 0.25, 0.75]
    t[3] = np.linspace(0.05, 0.9, ROUGH_W)
    return _rgba(np.repeat(t[..., None], 3, -1))


NMAP_W, NMAP_H = 8, 2


def normal_texture():
    """8x2 normal texels: (0.5, 0.5, 0.5) decodes to the zero vector, (0.5, 0.5, 0) to -z, (1, 0.5, 0.5) to the
    tangent, (0.5, 1, 0.5) to the bitangent, the rest to ordinary normals."""
    t = np.zeros((NMAP_H, NMAP_W, 3), f32)
    t[0, 0] = (0.5, 0.5, 0.5)
    t[0, 1] = (0.5, 0.5, 0.0)
    t[0, 2] = (1.0, 0.5, 0.5)
    t[0, 3] = (0.5, 1.0, 0.5)
    t[0, 4:] = [(0.5, 0.5, 1.0), (0.625, 0.5, 0.875), (0.5, 0.375, 0.9375), (0.75, 0.75, 0.75)]
    t[1] = np.random.default_rng([SEED, 77]).uniform(0.3, 0.7, (NMAP_W, 3))
    t[1, :, 2] = 0.9375
    return _rgba(t)


def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)


def _mat4(A, t=(0, 0, 0)):
    M = np.eye(4)
    M[:3, :3] = A
    M[:3, 3] = t
    return [float(f32(v)) for v in M.reshape(-1)]


TRANSFORMS = {  # the 16 values of a light's "transform"
    "identity": _mat4(np.eye(3)),
    "rotation": _mat4(_rot((1, 2, 3), 37.0), (0.7, -1.3, 2.1)),
    "scale": _mat4(np.diag([2.0, 0.5, 3.0]), (-1.0, 0.5, 0.25)),
    "shear": _mat4(np.array([[1.0, 0.4, 0.3], [0.0, 1.0, 0.6], [0.2, 0.0, 1.0]]), (0.3, 0.2, -0.4)),
}


def _session(integrator=None):
    s = {"imageWidth": 16, "imageHeight": 16, "bucketSize": 16, "spp": 1, "bounces": 2, "filterWidth": 2,
         "rougheningFactor": 0}
    if integrator:
        s["integrator"] = integrator
    return s


_CAM = [1, 0, 0, 0, 0, 0, -1, -5, 0, 1, 0, 0, 0, 0, 0, 1]


def _write(d, name, scene):
    path = os.path.join(d, name + ".json")
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
    return path


def _tex(d, name, arr):
    p = os.path.join(d, name + ".exr")
    scenes.write_texture(p, arr)
    return {"type": "texture", "filePath": p}


def area_lights():
    out = []
    for tname, T in TRANSFORMS.items():
        for r in (1e-3, 1.0, 1e3):
            out.append({"type": "disk", "radius": r, "Le": [1.0, 0.9, 0.8], "intensity": 3.0, "transform": T})
        for ratio in (1e-3, 0.5, 0.999):
            r = {"identity": 1.0, "rotation": 1e3, "scale": 1e-3, "shear": 1.0}[tname]
            out.append({"type": "ring", "radius": r, "innerRadius": float(f32(r) * f32(ratio)), "Le": [0.5, 0.7, 1.0],
                        "intensity": 2.0, "transform": T})
    return out


def write_scene(name, d):
    os.makedirs(d, exist_ok=True)
    tri = _tri_geo(os.path.join(d, "tri.geo"))
    disk = {"type": "disk", "radius": 0.5, "Le": [1, 1, 1], "intensity": 10.0, "transform": TRANSFORMS["rotation"]}
    mesh = lambda mat: {"filePath": tri, "material": mat}  # noqa: E731
    lam = {"type": "lambert", "rho_d": [0.5, 0.6, 0.7]}
    if name == "lights":
        lights = area_lights()
        lights.append({"type": "disk", "radius": 1.0, "Le": _tex(d, "le", env_texture("equal_row")), "intensity": 1.5,
                       "transform": TRANSFORMS["shear"]})
        lights.append({"type": "environment", "Le": _tex(d, "sky", env_texture("sky")), "intensity": 1.25})
        lights.append({"type": "environment", "Le": [0.8, 0.85, 1.0], "intensity": 0.75})
        return _write(d, name, {"renderSessions": [_session()], "camera": {"fov": 30.0, "transform": _CAM},
                                "meshes": [mesh(lam)], "lights": lights})
    if name.startswith("env_"):
        lights = [{"type": "environment", "Le": _tex(d, "map", env_texture(name[4:])), "intensity": 1.5}]
        return _write(d, name, {"renderSessions": [_session()], "camera": {"fov": 30.0, "transform": _CAM},
                                "meshes": [mesh(lam)], "lights": lights})
    if name in MEDIA:
        grid, bmin, bmax = MEDIA[name]
        rng = np.random.default_rng([SEED, SCENES.index(name)])
        vol = os.path.join(d, "medium.vol")
        scenes.write_vol(vol, bmin, bmax, rng.uniform(0.1, 1.0, grid).astype(f32))
        medium = {"filePath": vol, "Le": [2.0, 1.2, 0.4], "sigma_a": 1.5, "sigma_s": 3.0}
        lights = [{"type": "environment", "Le": _tex(d, "sky", env_texture("sky")), "intensity": 1.0}]
        return _write(d, name, {"renderSessions": [_session("volume")],
                                "camera": {"fov": 30.0, "transform": _CAM, "medium": medium}, "meshes": [], "lights": lights})
    if name == "mat_diffuse":
        mats = [lam, {"type": "lambert", "rho_d": [0.1, 0.2, 0.9]}]
        lights = [disk, {"type": "disk", "radius": 1e-3, "Le": [1, 1, 1], "intensity": 5.0, "transform": TRANSFORMS["scale"]}]
    elif name == "mat_glass":
        mats = [lam, {"type": "glass", "rho_s": [1, 1, 1], "tau": [0.9, 0.95, 1.0], "eta": 1.5, "roughness": 0.0},
                {"type": "glass", "rho_s": [0.9, 0.8, 0.7], "tau": [1.0, 0.6, 0.6], "eta": 1.33, "roughness": 0.15},
                {"type": "glass", "rho_s": [1, 1, 1], "tau": [1, 1, 1], "eta": 1.2, "roughness": 0.01}]
        lights = [disk, {"type": "disk", "radius": 1e3, "Le": [1, 1, 1], "intensity": 5.0, "transform": TRANSFORMS["shear"]}]
    elif name == "mat_envtex":
        albedo = _tex(d, "albedo", env_texture("zero_rows"))
        mats = [{"type": "lambert", "rho_d": albedo},
                {"type": "lambert", "rho_d": albedo, "normal": _tex(d, "nmap", normal_texture())},
                {"type": "plastic", "rho_d": albedo, "rho_s": [1, 1, 1], "eta": 1.5, "roughness": _tex(d, "rough", rough_texture()),
                 "normal": _tex(d, "nmap", normal_texture())},
                {"type": "plastic", "rho_d": [0.1, 0.3, 0.6], "rho_s": [0.9, 0.9, 0.9], "eta": 1.5, "roughness": 0.0}]
        lights = [{"type": "environment", "Le": _tex(d, "sky", env_texture("sky")), "intensity": 1.5}]
    else:  # materials: every kind, constant and textured
        albedo, rough, nmap = _tex(d, "albedo", env_texture("zero_rows")), _tex(d, "rough", rough_texture()), _tex(d, "nmap", normal_texture())
        etat = _tex(d, "eta", _rgba(np.full((2, 2, 3), 1.5, f32) + np.arange(4, dtype=f32).reshape(2, 2, 1) * f32(0.125)))
        mats = [lam,
                {"type": "lambert", "rho_d": albedo, "normal": nmap},
                {"type": "specular", "rho_s": [0.9, 0.9, 0.9], "eta": 8192},
                {"type": "specular", "rho_s": albedo, "eta": etat, "normal": nmap},
                {"type": "glass", "rho_s": [1, 1, 1], "tau": [0.9, 0.95, 1.0], "eta": 1.5, "roughness": 0.0},
                {"type": "glass", "rho_s": albedo, "tau": albedo, "eta": etat, "roughness": rough, "normal": nmap},
                {"type": "glossy", "rho_s": [0.95, 0.64, 0.54], "eta": 1.8, "roughness": 0.01},
                {"type": "glossy", "rho_s": albedo, "eta": etat, "roughness": rough, "normal": nmap},
                {"type": "plastic", "rho_d": [0.1, 0.3, 0.6], "rho_s": [1, 1, 1], "eta": 1.5, "roughness": 0.0316},
                {"type": "plastic", "rho_d": albedo, "rho_s": albedo, "eta": etat, "roughness": rough, "normal": nmap}]
        lights = [disk]
    return _write(d, name, {"renderSessions": [_session()], "camera": {"fov": 30.0, "transform": _CAM},
                            "meshes": [mesh(m) for m in mats], "lights": lights})


# ------------------------------------------------------------------------------------------------ float32 pieces
def _vm(v, m):
    """vec4 * mat4 as dmath.h vec_mul_mat, float32."""
    m = np.asarray(m, f32)
    v = np.asarray(v, f32)
    return np.array([((m[4 * i] * v[0] + m[4 * i + 1] * v[1]) + m[4 * i + 2] * v[2]) + m[4 * i + 3] * v[3] for i in range(4)], f32)


def _dot(a, b):  # GLM's dot(vec3) order, float32
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def light_frame(L):
    """center, n of an area light (disklight.cpp's per-call constants), float32, and a float64 orthonormal basis
    (a, b) of its plane."""
    c = _vm([0, 0, 0, 1], L.m)[:3]
    n = _vm([0, 0, -1, 0], L.m)[:3]
    n64 = n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
    a = np.cross(n64, [0.3, -0.5, 0.8])
    a /= np.linalg.norm(a)
    return c, n, a, np.cross(n64, a)


def area_terms(L, p, wi):
    """What area_pdf forms before its tests, float32 in its operation order: dot(wi, n), t, dist."""
    c, n, _, _ = light_frame(L)
    p, wi = np.asarray(p, f32), np.asarray(wi, f32)
    with np.errstate(all="ignore"):
        dn = _dot(wi, n)
        t = (f32(_dot(c, n)) - _dot(p, n)) / dn
        c2p = (p + wi * t[:, None]) - c
        dist = c2p[:, 0] * c2p[:, 0] + c2p[:, 1] * c2p[:, 1] + c2p[:, 2] * c2p[:, 2]
    return dn, t, dist


def env_tables(rgb):
    """mpdf and mcdf of the Piecewise2DDistribution of a texture (texturepattern.cpp:3-70), float32 in its
    operation order, from (H, W, >= 3) texels (top row first): the half bits a scene loaded (uint16) or their
    float32 values."""
    rgb = rgb.view(np.float16) if rgb.dtype == np.uint16 else rgb
    t = np.abs(rgb.astype(f32)[::-1, :, :3])
    H, W = t.shape[:2]
    tex = (t[..., 0] + t[..., 1]) + t[..., 2]
    mpdf = np.cumsum(tex, axis=1, dtype=f32)[:, -1] * (f32(1) / f32(W))
    fint = np.cumsum(mpdf, dtype=f32)[-1] * (f32(1) / f32(H))
    mpdf = mpdf * (f32(1) / fint)
    mcdf = np.concatenate([[f32(0)], np.cumsum(mpdf[:-1] * (f32(1) / f32(H)), dtype=f32)]).astype(f32)
    return mpdf, mcdf


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class Sets:
    """Record sets of one op: add(class, records) and all() -> (records, class index per record, class names)."""

    def __init__(self):
        self.parts = []

    def add(self, cls, x):
        x = np.ascontiguousarray(x, f32)
        if len(x):
            self.parts.append((cls, x))

    def all(self):
        names = sorted({c for c, _ in self.parts})
        x = np.concatenate([p for _, p in self.parts]) if self.parts else records(0)
        cls = np.concatenate([np.full(len(p), names.index(c)) for c, p in self.parts]) if self.parts else np.zeros(0, int)
        return x, cls, names


# ------------------------------------------------------------------------------------------------ record sets
def tex_records(sc, rng):
    s = Sets()
    for ti, tex in enumerate(sc.textures()):
        h, w = tex.shape[:2]

        def rec(su, sv, cls):
            su, sv = np.broadcast_arrays(np.asarray(su, f32), np.asarray(sv, f32))
            x = records(su.size)
            x[:, 0] = u32(np.full(su.size, ti))
            x[:, 1], x[:, 2] = su.ravel(), sv.ravel()
            x[:, 3] = u32(np.arange(su.size) & 1)  # is_roughness off and on
            s.add(cls, x)

        other = rng.uniform(0, 1, 64).astype(f32)
        lo = np.concatenate([edges(0.0001), [-INF, -1.0, -0.0, 0.0, 1e-45, 1e-30]]).astype(f32)
        hi = np.concatenate([edges(0.9999), [ONE_BELOW, 1.0, 2.0, INF]]).astype(f32)
        for e, cls in ((lo, "clamp_low"), (hi, "clamp_high")):
            rec(np.repeat(e, 8), np.resize(other, len(e) * 8), cls)
            rec(np.resize(other, len(e) * 8), f32(1) - np.repeat(e, 8), cls + "_flipped")
        # the 1 - sv flip itself: sv whose complement rounds onto a clamp
        flip = np.concatenate([edges(f32(1) - f32(0.9999)), edges(f32(1) - f32(0.0001)), edges(1.0), [0.0, -0.0, 1e-8, 6e-8]]).astype(f32)
        rec(np.resize(other, len(flip) * 4), np.repeat(flip, 4), "flip")
        # texel index (int)((float)w * u) on cell borders
        ku = np.concatenate([edges(f32(k) / f32(w)) for k in np.unique(np.linspace(0, w, min(w, 16) + 1).astype(int))])
        kv = np.concatenate([edges(f32(k) / f32(h)) for k in np.unique(np.linspace(0, h, min(h, 16) + 1).astype(int))])
        ru, rv = max(2, -(-32 // len(ku))), max(2, -(-32 // len(kv)))
        rec(np.repeat(ku, ru), np.resize(other, len(ku) * ru), "texel_border")
        rec(np.resize(other, len(kv) * rv), f32(1) - np.repeat(kv, rv), "texel_border")
        rec(np.full(40, np.nan), np.resize(other, 40), "nan_coordinate")
        rec(np.resize(other, 40), np.full(40, np.nan), "nan_coordinate")
        nf = max(64, N_FILL // max(1, len(sc.textures())))
        rec(rng.uniform(-0.5, 1.5, nf), rng.uniform(-0.5, 1.5, nf), "fill")
    return s


def env_pdf_records(sc, rng):
    s = Sets()
    texs = sc.textures()
    for li, L in enumerate(sc.lights()):
        if L.type != nart_amd.api.LIGHT_ENVIRONMENT:
            continue
        h, w = texs[L.Le.texture].shape[:2] if L.Le.type == nart_amd.api.PTN_TEXTURE else (4, 4)

        def rec(a, b, cls):
            a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
            x = records(a.size)
            x[:, 0] = u32(np.full(a.size, li))
            x[:, 1], x[:, 2] = a.ravel(), b.ravel()
            s.add(cls, x)

        other = rng.uniform(0, 1, 64).astype(f32)
        hi = np.concatenate([edges(0.9999), [ONE_BELOW, 1.0, 2.0, INF, np.nan]]).astype(f32)
        rec(np.repeat(hi, 6), np.resize(other, len(hi) * 6), "clamp")
        rec(np.resize(other, len(hi) * 6), np.repeat(hi, 6), "clamp")
        ku = np.concatenate([edges(f32(k) / f32(w)) for k in np.unique(np.linspace(0, w, min(w, 16) + 1).astype(int))])
        kv = np.concatenate([edges(f32(k) / f32(h)) for k in np.unique(np.linspace(0, h, min(h, 16) + 1).astype(int))])
        ru, rv = max(2, -(-32 // len(ku))), max(2, -(-32 // len(kv)))
        rec(np.clip(np.repeat(ku, ru), 0, None), np.resize(other, len(ku) * ru), "cell_border")
        rec(np.resize(other, len(kv) * rv), np.clip(np.repeat(kv, rv), 0, None), "cell_border")
        # a hair below 0 stays in cell 0 (the x86 conversion truncates towards zero); -1 cell and beyond run off
        neg = np.array([-0.0, -1e-45, -1e-30, -1e-8, -0.5 / w, -0.999 / w], f32)
        rec(np.repeat(neg, 8), np.resize(other, 48), "below_zero")
        rec(np.resize(other, 48), np.repeat(np.array([-0.0, -1e-45, -1e-30, -1e-8, -0.5 / h, -0.999 / h], f32), 8), "below_zero")
        if L.Le.type == nart_amd.api.PTN_TEXTURE:
            off = np.array([-1.0 / w, -1.5, -2.0, -1e9, -INF], f32)
            rec(np.repeat(off, 8), np.resize(other, 40), "off_table")
            rec(np.resize(other, 40), np.repeat(np.array([-1.0 / h, -1.5, -2.0, -1e9, -INF], f32), 8), "off_table")
        rec(rng.uniform(0, 1, N_FILL), rng.uniform(0, 1, N_FILL), "fill")
    return s


def _li_rec(li, p, wi, want=1, pdf=0.0, tmax=INF):
    p, wi = np.asarray(p, f32).reshape(-1, 3), np.asarray(wi, f32).reshape(-1, 3)
    x = records(len(p))
    x[:, 0] = u32(np.full(len(p), li))
    x[:, 1:4], x[:, 4:7] = p, wi
    x[:, 7] = u32(np.broadcast_to(np.asarray(want, np.uint32), (len(p),)))
    x[:, 8] = np.nan
    x[:, 9], x[:, 10] = pdf, tmax
    return x


def _presets(rng, n):
    """(want pdf, preset pdf, preset tMax): both integrators preset pdf 0 and tMax inf; a sentinel pdf and a
    finite tMax show what a miss leaves alone."""
    return rng.integers(0, 2, n), np.where(rng.integers(0, 2, n) == 1, SENTINEL, f32(0)), np.where(rng.integers(0, 3, n) == 0, f32(123.5), INF)


def light_li_records(sc, rng):
    s = Sets()
    for li, L in enumerate(sc.lights()):
        if L.type == nart_amd.api.LIGHT_ENVIRONMENT:
            def add(cls, wi):
                wi = np.asarray(wi, f32).reshape(-1, 3)
                want, pdf, tm = _presets(rng, len(wi))
                s.add(cls, _li_rec(li, rng.uniform(-1, 1, (len(wi), 3)), wi, want, pdf, tm))
            z = np.concatenate([edges(1.0), edges(-1.0)])
            xy = rng.uniform(-1, 1, (8, 2)).astype(f32) * f32(1e-4)
            add("pole", [(a, b, c) for c in z for a, b in np.concatenate([xy, [(0, 0), (-0.0, 0.0), (0.0, -0.0), (1e-30, 0)]])])
            zs = rng.uniform(-0.9, 0.9, 12).astype(f32)
            tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-30, -1e-30, 1e-8, -1e-8], f32)
            add("phi_pi", [(-1.0, y, c) for y in tiny for c in zs])      # atan2 = +-pi: phi = 2 pi or 0
            add("phi_zero", [(1.0, y, c) for y in tiny for c in zs])     # atan2 = +-0: phi = pi
            u = _unit(rng, 96)
            add("unnormalised", np.concatenate([u * 1e-3, u * 0.5, u * 0.999]))
            add("beyond_unit", u[:48] * np.where(np.abs(u[:48, 2:3]) > 0.5, 2.5, 1.0))  # |wi.z| > 1 where it can be: acosf is NaN
            add("fill", _unit(rng, N_FILL))
            continue
        c, n, a, b = light_frame(L)
        r = float(L.radius)
        ri = float(L.inner_radius)
        c64, n64 = c.astype(np.float64), n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))

        def toward(rho, k, tscale=None):
            """k records whose hit point lies at radius rho (array) from the centre: p = hit - wi * t."""
            phi = rng.uniform(0, 2 * np.pi, k)
            hit = c64 + (np.cos(phi)[:, None] * a + np.sin(phi)[:, None] * b) * np.asarray(rho)[:, None]
            wi = -n64 + 0.6 * _unit(rng, k)   # dot(wi, n) < 0
            wi /= np.linalg.norm(wi, axis=1, keepdims=True)
            t = rng.uniform(0.5, 2.0, k) * (r if tscale is None else tscale)
            return (hit - wi * t[:, None]).astype(f32), wi.astype(f32)

        def add(cls, p, wi, keep=None):
            p, wi = np.asarray(p, f32).reshape(-1, 3), np.asarray(wi, f32).reshape(-1, 3)
            if keep is not None:
                p, wi = p[keep], wi[keep]
            want, pdf, tm = _presets(rng, len(p))
            s.add(cls, _li_rec(li, p, wi, want, pdf, tm))

        # dist at r2 (and ri2) and on the nearest floats on either side: hit points within a few ulps of the rim,
        # kept where area_pdf's own float32 dist lands on the target
        for rim, tag in ((r, "r2"),) + (((ri, "ri2"),) if L.type == nart_amd.api.LIGHT_RING else ()):
            k = 6000
            p, wi = toward(rim * (1.0 + rng.integers(-6, 7, k) * 2.0 ** -25), k)
            _, _, dist = area_terms(L, p, wi)
            target = f32(rim) * f32(rim)
            for e, side in zip(edges(target), ("below", "at", "above")):
                add("%s_%s" % (tag, side), p, wi, np.nonzero(dist == e)[0][:64])
            add("%s_near" % tag, p[:256], wi[:256])
        # dot(wi, n) of +-0 and of either sign next to 0: directions in the plane, then tipped out of it
        inp = (np.cos(np.linspace(0, 6, 48))[:, None] * a + np.sin(np.linspace(0, 6, 48))[:, None] * b)
        pp = (c64 + 0.3 * r * _unit(rng, 48) + n64 * 0.0).astype(f32)
        for cls, tip in (("grazing", 0.0), ("grazing_front", -1e-7), ("grazing_back", 1e-7), ("grazing_front", -1e-30), ("grazing_back", 1e-30)):
            add(cls, pp, (inp + tip * n64).astype(f32))
        ax = np.array([(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (1, 1, 0), (1, 0, 0.0), (0, 1, -0.0), (3, -2, 0)], f32)
        add("grazing", np.repeat(pp[:8], 8, 0), np.tile(ax, (8, 1)))  # exact zeros where n is along z
        # t next to 0, p on the plane and at the centre
        k = 96
        p, wi = toward(rng.uniform(0, 1.2, k) * r, k, tscale=0.0)
        add("on_plane", p, wi)
        add("at_centre", np.tile(c, (48, 1)), toward(np.zeros(48), 48)[1])
        p, wi = toward(rng.uniform(0, 1.2, k) * r, k, tscale=1e-6 * max(r, 1e-3))
        add("t_near_zero", p, wi)
        add("t_near_zero", p, -wi)  # behind the plane: t < 0
        p, wi = toward(rng.uniform(0, 1.5, 192) * r, 192)
        add("unnormalised", np.concatenate([p[:96], p[96:]]), np.concatenate([wi[:96] * f32(1e-3), wi[96:] * f32(1e3)]))
        nf = max(128, N_FILL // len(sc.lights()))
        p, wi = toward(rng.uniform(0, 1.5, nf) * r, nf)
        add("fill", p, wi)
    return s


def light_sample_records(sc, rng):
    s = Sets()
    texs = sc.textures()
    for li, L in enumerate(sc.lights()):
        def rec(cls, p, smp, pdf=None):
            smp = np.asarray(smp, f32).reshape(-1, 2)
            x = records(len(smp))
            x[:, 0] = u32(np.full(len(smp), li))
            x[:, 1:4] = np.asarray(p, f32).reshape(-1, 3)
            x[:, 4:6] = smp
            x[:, 9] = np.where(np.arange(len(smp)) & 1, SENTINEL, f32(0)) if pdf is None else pdf
            x[:, 10] = np.where(np.arange(len(smp)) % 3 == 0, f32(123.5), INF)
            s.add(cls, x)

        corner = np.array([(a, b) for a in (0.0, ONE_BELOW, 0.5, 1e-8) for b in (0.0, ONE_BELOW, 0.5, 1e-8)], f32)
        if L.type == nart_amd.api.LIGHT_ENVIRONMENT:
            n0 = np.zeros(3, f32)
            rec("sample_edges", np.tile(n0, (64, 1)), np.tile(corner, (4, 1)))
            if L.Le.type == nart_amd.api.PTN_TEXTURE:
                mpdf, mcdf = env_tables(texs[L.Le.texture])
                h = len(mpdf)
                # sample.y on every row boundary of the marginal CDF and next to it
                sy = np.unique(np.clip(np.concatenate([edges(v) for v in mcdf] + [edges(1.0)]), 0, ONE_BELOW)).astype(f32)
                sy = np.resize(sy, max(len(sy), 96))
                rec("row_border", np.tile(n0, (len(sy), 1)), np.stack([np.resize(rng.uniform(0, 1, 7).astype(f32), len(sy)), sy], 1))
                zero = np.nonzero(mpdf == 0)[0]
                if len(zero):  # aimed at the zero rows: the row vc lands in is v = (uint32)(vc * h)
                    for j in zero:
                        sy = np.concatenate([edges(mcdf[j]), edges(mcdf[min(j + 1, h - 1)]), [ONE_BELOW]]).astype(f32)
                        sy = np.clip(sy, 0, ONE_BELOW)
                        rec("zero_row_aim", np.tile(n0, (len(sy) * 4, 1)), np.stack([np.resize(rng.uniform(0, 1, 4).astype(f32), len(sy) * 4), np.repeat(sy, 4)], 1))
                bright = [j for j in range(h) if texs[L.Le.texture].shape[1] > 1 and
                          (np.abs(texs[L.Le.texture].view(np.float16)[h - 1 - j, :, :3].astype(f32)).sum(1) > 0).sum() == 1]
                for j in bright:
                    lo, hi = float(mcdf[j]), float(mcdf[j + 1]) if j + 1 < h else 1.0
                    sy = rng.uniform(lo, hi, 96).astype(f32)
                    rec("one_texel_row", np.tile(n0, (96, 1)), np.stack([np.concatenate([rng.uniform(0, 1, 80), np.resize(corner[:, 0], 16)]).astype(f32), sy], 1))
            rec("fill", np.tile(n0, (N_FILL, 1)), rng.uniform(0, 1, (N_FILL, 2)))
            continue
        c, n, a, b = light_frame(L)
        r = float(L.radius)
        c64, n64 = c.astype(np.float64), n.astype(np.float64) / np.linalg.norm(n.astype(np.float64))
        front = lambda k: (c64 - n64 * rng.uniform(0.2, 3, (k, 1)) * max(r, 1e-2) + 0.5 * r * _unit(rng, k)).astype(f32)  # noqa: E731
        rec("sample_edges", front(64), np.tile(corner, (4, 1)))
        rec("behind", (2 * c64 - front(96)).astype(f32), rng.uniform(0, 1, (96, 2)))   # wiDotN <= 0
        inpl = (c64 + (rng.uniform(-2, 2, (96, 1)) * a + rng.uniform(-2, 2, (96, 1)) * b) * r).astype(f32)
        rec("on_plane", inpl, rng.uniform(0, 1, (96, 2)))
        rec("at_centre", np.tile(c, (48, 1)), rng.uniform(0, 1, (48, 2)))
        nf = max(128, N_FILL // len(sc.lights()))
        rec("fill", front(nf), rng.uniform(0, 1, (nf, 2)))
    return s


B_LAMBERT, B_SPECULAR, B_SPECDIEL, B_DIEL, B_TS = range(5)
THRESHOLDS = (f32(0.0001), f32(0.001))


def _tweaks_for(alpha, thr):
    """alphaTweak values that put ap = 1 - (1 - alpha) * tweak on the two multiples of 2^-24 around thr (ap is a
    difference from 1, so those are the nearest values it can take on either side), and a few steps further out."""
    alpha = f32(alpha)
    out = []
    k0 = int(np.floor(float(thr) * 2 ** 24))
    for k in (k0 - 3, k0 - 1, k0, k0 + 1, k0 + 2, k0 + 4):
        t0 = f32((1.0 - k * 2.0 ** -24) / (1.0 - float(alpha)))
        cand = t0
        for _ in range(6):
            cand = np.nextafter(cand, f32(0))
        for _ in range(13):
            ap = f32(1) - ((f32(1) - alpha) * cand)
            if ap == f32(k * 2.0 ** -24):
                out.append(cand)
                break
            cand = np.nextafter(cand, f32(2))
    return out


def bsdf_records(sc, rng):
    s = Sets()
    texs = sc.textures()
    for mi, m in enumerate(sc.materials()):
        def rec(cls, st, sn, dpds, tweak):
            st = np.asarray(st, f32).reshape(-1, 2)
            k = len(st)
            x = records(k)
            x[:, 0] = u32(np.full(k, mi))
            x[:, 1:3] = st
            x[:, 3:6] = np.broadcast_to(np.asarray(sn, f32), (k, 3))
            x[:, 6:9] = np.broadcast_to(np.asarray(dpds, f32), (k, 3))
            x[:, 9] = np.broadcast_to(np.asarray(tweak, f32), (k,))
            s.add(cls, x)

        def frame(k):
            sn = _unit(rng, k)
            return sn.astype(f32), (np.cross(sn, _unit(rng, k)) + 0.2 * sn).astype(f32)

        def centre(i, j, w, h):  # the st that tex_fetch maps to texel (row j, column i)
            return (f32(i) + f32(0.5)) / f32(w), f32(1) - (f32(j) + f32(0.5)) / f32(h)

        textured = m.alpha.type == nart_amd.api.PTN_TEXTURE
        kind = m.type
        thr = THRESHOLDS[1] if kind == nart_amd.api.MAT_PLASTIC else THRESHOLDS[0]
        if kind != nart_amd.api.MAT_LAMBERT:
            # ap on either side of the kind's threshold: from the alpha the material has at a texel centre
            cells = [(i, j) for j in range(ROUGH_H) for i in range(ROUGH_W)] if textured else [(0, 0)]
            for i, j in cells:
                if kind == nart_amd.api.MAT_SPECULAR:
                    alpha = f32(0)
                elif textured:
                    t = texs[m.alpha.texture].view(np.float16)[j, i, 0].astype(f32)
                    alpha = t * t
                else:
                    alpha = f32(m.alpha.value[0])
                if float(alpha) >= 0.5:  # 1 - alpha then has a coarser grid than ap's: no tweak lands on the targets
                    continue
                tw = _tweaks_for(alpha, thr)
                if not tw:
                    continue
                k = 2 if textured else 12
                sn, dp = frame(len(tw) * k)
                st = np.tile(centre(i, j, ROUGH_W, ROUGH_H), (len(tw) * k, 1)) if textured else rng.uniform(0, 1, (len(tw) * k, 2))
                rec("threshold", st, sn, dp, np.repeat(np.array(tw, f32), k))
        if m.has_normal and kind != nart_amd.api.MAT_GLASS:
            for i, cls in ((0, "normal_zero"), (1, "normal_minus_z"), (2, "normal_tangent"), (3, "normal_bitangent")):
                sn, dp = frame(40)
                rec(cls, np.tile(centre(i, 0, NMAP_W, NMAP_H), (40, 1)), sn, dp, rng.uniform(0, 1, 40))
        sn, dp = frame(40)
        rec("dpds_parallel", rng.uniform(0, 1, (40, 2)), sn, sn * rng.choice([1.0, -1.0, 2.5, 1e-3], (40, 1)).astype(f32), rng.uniform(0, 1, 40))
        sn, dp = frame(40)
        rec("sn_not_unit", rng.uniform(0, 1, (40, 2)), sn * rng.choice([0.5, 3.0, 1e-3, 1e3], (40, 1)).astype(f32), dp, rng.uniform(0, 1, 40))
        rec("tweak_edges", rng.uniform(0, 1, (48, 2)), *frame(48), np.resize(np.array([0.0, 1.0, ONE_BELOW, 0.5, 2.0, -1.0], f32), 48))
        nf = max(256, N_FILL // len(sc.materials()))
        rec("fill", rng.uniform(-0.25, 1.25, (nf, 2)), *frame(nf), rng.uniform(0, 1, nf))
    return s


def dg_records(sc, rng):
    s = Sets()
    rx, ry, rz = sc.medium()["res"]

    def rec(cls, p):
        x = records(len(p))
        x[:, 0:3] = np.asarray(p, f32).reshape(-1, 3)
        s.add(cls, x)

    def mix(vals, k=None):
        """Points with one, two or all three coordinates from vals, the others from [0, 1)."""
        vals = np.asarray(vals, f32)
        k = k or max(96, 6 * len(vals))
        p = rng.uniform(0, 1, (k, 3)).astype(f32)
        which = rng.integers(1, 8, k)
        for a in range(3):
            on = (which >> a) & 1 == 1
            p[on, a] = vals[rng.integers(0, len(vals), on.sum())]
        return p

    rec("zero", mix([0.0, -0.0, 1e-45, 1e-30]))
    rec("clamp_high", mix(np.concatenate([edges(0.999), [ONE_BELOW, 1.0]])))
    rec("below_zero", mix([-1e-45, -1e-8, -0.5, -1e9, -INF]))
    rec("above_one", mix([np.nextafter(f32(1), f32(2)), 1.5, 1e9, INF]))
    planes = []
    for a, res in enumerate((rx, ry, rz)):
        ks = np.unique(np.linspace(0, res - 1, min(res, 24)).astype(int))
        v = np.concatenate([edges(f32(k) / f32(res - 1)) for k in ks])
        p = rng.uniform(0, 1, (len(v) * 3, 3)).astype(f32)
        p[:, a] = np.repeat(v, 3)
        planes.append(p)
    rec("lattice_plane", np.concatenate(planes))
    rec("fill", rng.uniform(0, 1, (N_FILL, 3)))
    return s


def walk_records(sc, rng):
    s = Sets()
    med = sc.medium()
    lo, hi = med["bounds_min"].astype(np.float64), med["bounds_max"].astype(np.float64)
    size, mid = hi - lo, (hi + lo) / 2

    def rec(cls, o, d):
        o, d = np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3)
        x = records(len(o))
        x[:, 0:3], x[:, 3:6] = o, d
        s.add(cls, x)

    inside = lambda k: lo + size * rng.uniform(0.05, 0.95, (k, 3))  # noqa: E731
    outside = lambda k: mid + size * _unit(rng, k) * rng.uniform(1.0, 3.0, (k, 1))  # noqa: E731

    def on(dims, k):
        """Points with `dims` coordinates exactly on a bound: 1 a face, 2 an edge, 3 a corner."""
        p = inside(k)
        for i in range(k):
            for a in rng.permutation(3)[:dims]:
                p[i, a] = (lo, hi)[rng.integers(0, 2)][a]
        return p

    k = 96
    rec("inside", inside(k), _unit(rng, k))
    o = outside(k)
    rec("outside_toward", o, inside(k) - o)
    rec("pointing_away", o, o - inside(k))
    for dims, cls in ((1, "on_face"), (2, "on_edge"), (3, "at_corner")):
        p = on(dims, k)
        rec(cls, p, np.concatenate([_unit(rng, k // 2), (mid - p[k // 2:])]))
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1e-30, -1e-30], f32)
    d = _unit(rng, 192).astype(f32)
    which = rng.integers(1, 7, 192)  # one or two components replaced
    for a in range(3):
        sel = (which >> a) & 1 == 1
        d[sel, a] = special[rng.integers(0, len(special), sel.sum())]
    rec("zero_component", np.concatenate([inside(96), outside(96)]), d)
    # grazing an edge or a corner: through a point on it, across the box's outside (tMin == tMax where it touches)
    for dims in (2, 3):
        p = on(dims, k)
        away = np.where(p == lo, -1.0, np.where(p == hi, 1.0, 0.0))
        t = np.cross(away, _unit(rng, k))
        t = np.where(np.linalg.norm(t, axis=1, keepdims=True) > 0, t, 1.0) * size
        rec("grazing", p - t * rng.uniform(0.5, 2.0, (k, 1)), t)
    axis = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1))
    rec("axis_on_face", on(1, k), axis)  # along or into a face from a point on one
    u = _unit(rng, k)
    rec("unnormalised", np.concatenate([inside(k // 2), outside(k // 2)]), np.concatenate([u[:k // 2] * 1e-3, -outside(k // 2) * 1e3 / np.max(size)]))
    o = np.concatenate([inside(N_FILL // 2), outside(N_FILL // 2)])
    rec("fill", o, np.concatenate([_unit(rng, N_FILL // 2), inside(N_FILL // 2) - o[N_FILL // 2:]]))
    return s


GENERATORS = {"tex_fetch": tex_records, "env_pdf": env_pdf_records, "light_li": light_li_records,
              "light_bound": light_li_records, "light_sample_li": light_sample_records, "create_bsdf": bsdf_records,
              "dg_lookup": dg_records, "medium_walk": walk_records}


def ops_of(sc):
    """The ops a scene can answer."""
    ops = []
    if sc.textures():
        ops.append("tex_fetch")
    if any(L.type == nart_amd.api.LIGHT_ENVIRONMENT for L in sc.lights()):
        ops.append("env_pdf")
    if sc.lights():
        ops += ["light_li", "light_bound", "light_sample_li"]
    if sc.materials():
        ops.append("create_bsdf")
    if sc.medium() is not None:
        ops += ["dg_lookup", "medium_walk"]
    return ops


# words of an answer that are compared (include/nart_hip.h; the rest are 0 on both sides)
WORDS = {"tex_fetch": 3, "env_pdf": 1, "light_li": 5, "light_bound": 5, "light_sample_li": 8, "create_bsdf": 32,
         "dg_lookup": 4, "medium_walk": 32}
# words that hold integers: compared as bits, never NaN
INT_WORDS = {"create_bsdf": (9, 10, 11, 21, 22), "dg_lookup": (3,), "medium_walk": (0, 1) + tuple(range(7, 32, 4))}

_PREPARED = {}


def prepared(name, directory):
    """Everything the tests of one scene share, computed once per process and changed by nobody: the scene, its
    oracle, the builds it fits and per op the records, the class of each, the oracle's answers and flags."""
    if name not in _PREPARED:
        import oracle
        sc = nart_amd.Scene(write_scene(name, os.path.join(directory, name)))
        orc = oracle.Oracle(sc)
        prep = {"scene": sc, "oracle": orc, "ops": {}}
        for op in ops_of(sc):
            rng = np.random.default_rng([SEED, SCENES.index(name), OPS.index("light_li" if op == "light_bound" else op)])
            x, cls, names = GENERATORS[op](sc, rng).all()
            want, flags = oracle.scene_eval(orc, op, x)
            prep["ops"][op] = {"x": x, "cls": cls, "classes": names, "want": want, "flags": flags}
        _PREPARED[name] = prep
    return _PREPARED[name]


def of_class(p, c):
    return p["cls"] == p["classes"].index(c) if c in p["classes"] else np.zeros(len(p["cls"]), bool)


def set_aside(op, p):
    """Records of a documented, named case the device does not emulate: none.  The one candidate, maj_next past
    majorant index 7 (RayMajorantIterator::Next indexing beyond the Medium object, undefined in the reference),
    cannot be listed: the index starts at 0 and grows by at most 1 per call, and a record lists at most
    NART_SCENE_WALK_SEGMENTS = 7 calls, so the largest index a listed segment uses is 6."""
    return np.zeros(len(p["x"]), bool)


def sendable(p):
    """The records that may go to the device: the oracle read no table out of bounds."""
    import oracle
    return (p["flags"] & oracle.SCENE_OOB) == 0


def compare(op, got, want):
    """Indices of the records whose device answer differs from the oracle's: bit for bit on every compared word
    where the oracle's float is not NaN, NaN where it is (x86 and the GPU differ in a generated NaN's sign and
    payload); integer words bit for bit."""
    g, w = got[:, :WORDS[op]], want[:, :WORDS[op]]
    nan = np.isnan(w)
    nan[:, [k for k in INT_WORDS.get(op, ()) if k < WORDS[op]]] = False
    bad = np.where(nan, ~np.isnan(g), g.view(np.uint32) != w.view(np.uint32))
    return np.nonzero(bad.any(axis=1) | (got[:, WORDS[op]:].view(np.uint32) != 0).any(axis=1))[0]


def nan_share(op, p):
    """Share of the sendable records with an oracle NaN in a compared float word."""
    w = p["want"][sendable(p)][:, :WORDS[op]].copy()
    w[:, [k for k in INT_WORDS.get(op, ()) if k < WORDS[op]]] = 0
    return float(np.isnan(w).any(axis=1).mean()) if len(w) else 0.0


def describe(op, p, got, idx, limit=5):
    lines = ["%s: %d of %d records differ" % (op, len(idx), len(p["x"]))]
    for i in idx[:limit]:
        k = np.nonzero(got[i].view(np.uint32) != p["want"][i].view(np.uint32))[0]
        lines.append("  record %d (%s) in %r\n    words %r device %r oracle %r" % (
            i, p["classes"][p["cls"][i]], p["x"][i, :11].tolist(), k.tolist(), got[i, k].tolist(), p["want"][i, k].tolist()))
    return "\n".join(lines)
