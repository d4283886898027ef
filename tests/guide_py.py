"""Restatement of the followed guides' chain (include/nart_hip.h, "Followed guides"; device/guide.h)
for tests/test_guide_restatement.py and tests/test_gpu_guides.py.

One step: given a segment's ray (o, d), the triangle it hit and the nested-dielectric list so far,
the list's verdict and eta_outer, whether the hit is followed, stepped through or the guide hit, the
next ray -- every operation in a chosen dtype, float64 as the yardstick and float32 in the device's
operation order (path.h fill_isect, create_bsdf, to_local, bxdf_sample_f, to_world) -- and the
records.  Barycentrics, the shading normal and the material tables are aov_py's; hits come from
oracle.trace.  walk() chains the steps from a camera ray with the bound of the analytic lights left
out (tmax = +inf): the device reports its own bound per segment, and the GPU tests check it there.

Not restated: normal maps (a followed surface with one raises; a guide hit's normal is then not
comparable and is flagged) and textured eta / alpha below the smooth threshold."""
import json
import os

import numpy as np

import aov_py
import nart_amd
import oracle
from nart_amd import scenes

NO_HIT = aov_py.NO_HIT
SHADOW_BIAS = np.float32(0.001)
FOLLOWED, STEPPED, GUIDE_HIT, MISS = "followed", "stepped", "guide", "miss"
A = nart_amd.api


def two_sphere_scene(directory):
    """Two overlapping smooth glass spheres in front of a Lambert wall, the nearer one (mesh 0,
    priority 3, eta 1.3) ahead of the farther (mesh 1, priority 2, eta 1.5): a ray through the middle
    enters mesh 0, meets mesh 1's surface inside it -- a lower-priority interface, stepped through --
    leaves mesh 0 inside mesh 1, and leaves mesh 1.  The disk light lies behind the camera."""
    os.makedirs(directory, exist_ok=True)
    scenes.write_geo(os.path.join(directory, "near.geo"), *scenes._uv_sphere((0.0, -0.3, 1.0), 0.5, 12, 24))
    scenes.write_geo(os.path.join(directory, "far.geo"), *scenes._uv_sphere((0.0, 0.3, 1.0), 0.5, 12, 24))
    scenes.write_geo(os.path.join(directory, "wall.geo"),
                     *scenes._uv_grid((-2.0, 2.0, -1.0), (4.0, 0, 0), (0, 0, 4.0), (0, -1, 0), 4))
    glass = lambda eta: {"type": "glass", "rho_s": [1, 1, 1], "tau": [1, 1, 1], "eta": eta, "roughness": 0}  # noqa: E731
    scene = {
        "renderSessions": [{"imageWidth": 48, "imageHeight": 36, "bucketSize": 16, "spp": 4, "bounces": 10,
                            "filterWidth": 2, "rougheningFactor": 0}],
        "camera": {"fov": 16.5, "transform": [1, 0, 0, 0, 0, 0, -1, -3.9, 0, 1, 0, 1, 0, 0, 0, 1]},
        "meshes": [{"filePath": os.path.join(directory, "near.geo"), "priority": 3, "material": glass(1.3)},
                   {"filePath": os.path.join(directory, "far.geo"), "priority": 2, "material": glass(1.5)},
                   {"filePath": os.path.join(directory, "wall.geo"),
                    "material": {"type": "lambert", "rho_d": [0.5, 0.4, 0.3]}}],
        "lights": [{"type": "disk", "radius": 0.5, "Le": [1, 1, 1], "intensity": 20.0,
                    "transform": [1, 0, 0, 0, 0, 1, 0, -6.0, 0, 0, 1, 1.0, 0, 0, 0, 1]}],
    }
    path = os.path.join(directory, "two_spheres.json")
    with open(path, "w") as f:
        json.dump(scene, f, indent=1)
    return path


class NestedList:
    """pathintegrator.cpp:7-36 and 123-142: the interfaces the chain is inside of, as (mesh, priority, eta)."""

    def __init__(self):
        self.e = []

    def valid(self, mesh, prio):
        """(IsectIsValid, eta_outer): false where a listed interface has a higher priority; eta_outer
        is the eta of the last entry that is not this mesh's own (1 without one)."""
        eta_outer = 1.0
        ok = all(prio >= p for _m, p, _e in self.e)
        if self.e:
            if self.e[-1][0] != mesh:
                eta_outer = self.e[-1][2]
            elif len(self.e) >= 2:
                eta_outer = self.e[-2][2]
        return ok, eta_outer

    def update(self, mesh, prio, eta):
        """Leaving removes the mesh's most recent entry, entering appends one."""
        for k in range(len(self.e) - 1, -1, -1):
            if self.e[k][0] == mesh:
                del self.e[k]
                return
        self.e.append((mesh, prio, float(eta)))

    def meshes(self):
        return [m for m, _p, _e in self.e]


class GuideScene:
    """The blob's tables as the chain needs them."""

    def __init__(self, scene):
        self.scene = scene
        self.tris = scene.triangles()
        self.mats = scene.materials()
        self.tri_mat = aov_py.tri_material(scene)
        n = scene.counts()["triangles"]
        self.tri_mesh = np.full(n, -1, np.int64)
        self.mesh_prio = []
        for i, (first, num, _material, prio) in enumerate(scene.meshes()):
            self.tri_mesh[first:first + num] = i
            self.mesh_prio.append(int(prio))
        self._tex_min = {}

    def _scalar(self, ptn):
        """A scalar pattern's float32 value; a texture gives its least texel (enough to tell rough
        from smooth)."""
        if ptn.type == A.PTN_CONSTANT:
            return np.float32(ptn.value[0])
        if ptn.texture not in self._tex_min:
            tex = self.scene.textures()[ptn.texture]
            self._tex_min[ptn.texture] = np.float32(tex[..., 0].view(np.float16).astype(np.float32).min())
        return self._tex_min[ptn.texture]

    def lobe(self, tri):
        """(kind, eta) of the BSDF create_bsdf builds at alphaTweak = 1: kind "mirror", "dielectric"
        (the two delta lobes the chain follows) or "other"; eta = bxdf_eta of the lobe Sample_f
        selects at s1 = 0 (0 for Lambert, plastic's first lobe)."""
        m = self.mats[self.tri_mat[tri]]
        one = np.float32(1)
        if m.type in (A.MAT_LAMBERT, A.MAT_PLASTIC):
            return "other", 0.0
        if m.eta.type != A.PTN_CONSTANT:
            raise NotImplementedError("textured eta")
        eta = float(np.float32(m.eta.value[0]))
        alpha = np.float32(0) if m.type == A.MAT_SPECULAR else self._scalar(m.alpha)
        ap = one - ((one - alpha) * one)
        if ap > np.float32(0.0001):
            return "other", eta
        if m.alpha.type != A.PTN_CONSTANT and m.type != A.MAT_SPECULAR:
            raise NotImplementedError("textured alpha below the smooth threshold")
        return ("dielectric" if m.type == A.MAT_GLASS else "mirror"), eta

    def has_normal_map(self, tri):
        return bool(self.mats[self.tri_mat[tri]].has_normal)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(x, y):
    return np.array([x[1] * y[2] - y[1] * x[2], x[2] * y[0] - y[2] * x[0], x[0] * y[1] - y[0] * x[1]], x.dtype)


def _normalize(v):
    s = v.dtype.type(1) / np.sqrt(_dot(v, v))
    return v * s


def hit_frame(T, o, d, dtype):
    """fill_isect and create_bsdf's frame without a normal map: p, gn, sn (= bs.n), n_t, n_b."""
    T, o, d = np.asarray(T, dtype), np.asarray(o, dtype), np.asarray(d, dtype)
    v0, v1, v2 = T[0:3], T[3:6], T[6:9]
    a = np.abs(d)
    major = (0 if a[0] > a[2] else 2) if a[0] > a[1] else (1 if a[1] > a[2] else 2)
    m0, m1 = (major + 1) % 3, (major + 2) % 3
    sz = dtype(1) / d[major]
    sx, sy = -d[m0] * sz, -d[m1] * sz
    pts = []
    for v in (v0, v1, v2):
        q = v - o
        pts.append((q[m0] + q[major] * sx, q[m1] + q[major] * sy))
    (p0x, p0y), (p1x, p1y), (p2x, p2y) = pts
    e0 = (p1x * p2y) - (p1y * p2x)
    e1 = (p2x * p0y) - (p2y * p0x)
    e2 = (p0x * p1y) - (p0y * p1x)
    inv_det = dtype(1) / (e0 + e1 + e2)
    p = ((v0 * e0 + v1 * e1) + v2 * e2) * inv_det
    u, v, w = aov_py.barycentrics(T, o, d, dtype)
    gn = _normalize(_cross(v1 - v0, v2 - v0))
    sn = (T[9:12] * u + T[12:15] * v) + T[15:18] * w
    uv0, uv1, uv2 = T[18:20], T[20:22], T[22:24]
    uv_det = ((uv0[0] - uv2[0]) * (uv1[1] - uv2[1])) - ((uv0[1] - uv2[1]) * (uv1[0] - uv2[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv_uv = dtype(1) / uv_det
        dpds = ((v0 - v2) * (uv1[1] - uv2[1]) + (v1 - v2) * (uv2[1] - uv0[1])) * inv_uv
        n_t = _normalize(dpds - sn * _dot(dpds, sn))
        n_b = _normalize(_cross(sn, n_t))
    return {"p": p, "gn": gn, "sn": sn, "n_t": n_t, "n_b": n_b}


def plane_distance(T, o, d, dtype):
    """The first-hit depth's t: (dot(v0, n) - dot(o, n)) / dot(d, n), n = cross(v1 - v0, v2 - v0)."""
    T, o, d = np.asarray(T, dtype), np.asarray(o, dtype), np.asarray(d, dtype)
    v0 = T[0:3]
    n = _cross(T[3:6] - v0, T[6:9] - v0)
    return (_dot(v0, n) - _dot(o, n)) / _dot(d, n)


def _sample_delta(kind, wo, eta_outer, eta, dtype):
    """bxdf_sample_f of the mirror and the smooth dielectric at sample = (1, 0), which is never < Fr:
    (wi, pdf > 0, transmissive, reflected by total internal reflection)."""
    if kind == "mirror":
        return np.array([-wo[0], -wo[1], wo[2]], dtype), True, False, False
    eta_o, eta_i = dtype(eta_outer), dtype(eta)
    if eta_o == eta_i:
        return -wo, False, True, False  # index-matched: pdf = 0
    if wo[2] < 0:
        eta_o, eta_i = eta_i, eta_o
    sin_o = np.sqrt(dtype(1) - (wo[2] * wo[2]))
    with np.errstate(divide="ignore", invalid="ignore"):  # (a stepped-through Lambert surface lists eta 0)
        ratio = eta_o / eta_i
    sin_i = ratio * sin_o
    if sin_i >= 1:
        return np.array([-wo[0], -wo[1], wo[2]], dtype), True, False, True
    n = np.array([0, 0, 1], dtype)
    a = wo - n * wo[2]
    c = (-a) * ratio
    dd = (-n) * np.sqrt(dtype(1) - (sin_i * sin_i))
    if wo[2] < 0:
        dd = dd * dtype(-1)
    return _normalize(c + dd), True, True, False


def step(gs, tri, o, d, nlist, k, max_follow, dtype):
    """One hit of the chain (steps 4-8 of the definition): the decision, the list's verdict, the next
    ray in `dtype`, and nlist updated in place as the chain updates it."""
    T = gs.tris[tri]
    mesh = int(gs.tri_mesh[tri])
    prio = gs.mesh_prio[mesh]
    ok, eta_outer = nlist.valid(mesh, prio)
    kind, eta = gs.lobe(tri)
    out = {"tri": int(tri), "mesh": mesh, "valid": ok, "eta_outer": eta_outer, "lobe": kind, "decision": GUIDE_HIT,
           "tir": False, "o": None, "d": None}
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    bias = dtype(SHADOW_BIAS)
    if k >= max_follow:
        return out
    if not ok:
        f = hit_frame(T, o, d, dtype)
        out.update(decision=STEPPED, o=f["p"] + d * bias, d=d)
        nlist.update(mesh, prio, eta)
        return out
    if kind == "other":
        return out
    if gs.has_normal_map(tri):
        raise NotImplementedError("a followed surface with a normal map")
    f = hit_frame(T, o, d, dtype)
    v = -d
    wo = _normalize(np.array([_dot(v, f["n_t"]), _dot(v, f["n_b"]), _dot(v, f["sn"])], dtype))
    wi, has_pdf, transmissive, tir = _sample_delta(kind, wo, eta_outer, eta, dtype)
    if not has_pdf:
        return out
    flip = dtype(1) if wi[2] > 0 else dtype(-1)
    world = _normalize((f["n_t"] * wi[0] + f["n_b"] * wi[1]) + f["sn"] * wi[2])
    out.update(decision=FOLLOWED, tir=tir, o=f["p"] + (f["gn"] * bias) * flip, d=world)
    if transmissive:
        nlist.update(mesh, prio, eta)
    return out


def albedo_value(gs, tri, o, d):
    """The guide hit's albedo: the constant pattern's value, or for a textured pattern the texel at
    TexturePattern's index (texturepattern.cpp:172-187) from the float64 st; near_edge where the
    scaled coordinate lies within 1e-3 of a texel boundary (float32 st may round across it)."""
    ptn = aov_py.albedo_pattern(gs.mats[gs.tri_mat[tri]])
    if ptn.type == A.PTN_CONSTANT:
        return np.float32(list(ptn.value)), False
    tex = gs.scene.textures()[ptn.texture]
    th, tw = tex.shape[:2]
    st = aov_py.surface_st(gs.tris[tri], o, d, np.float64)
    su = tw * min(max(st[0], 0.0001), 0.9999)
    sv = th * min(max(1.0 - st[1], 0.0001), 0.9999)
    near = min(abs(su - round(su)), abs(sv - round(sv))) < 1e-3
    return tex[int(sv), int(su), :3].view(np.float16).astype(np.float32), near


def walk(gs, orc, o, d, max_follow, dtype=np.float32, tmax=float("inf")):
    """The whole chain of one camera ray on the CPU: a list of step() results (a final {"decision":
    MISS} where a segment hits nothing), hits from oracle.trace, rays carried in `dtype` and handed
    to the oracle as float32."""
    nlist = NestedList()
    steps = []
    o, d = np.asarray(o, dtype), np.asarray(d, dtype)
    for k in range(max_follow + 1):
        tri = oracle.trace(orc, o.astype(np.float32), d.astype(np.float32), tmax)[0]
        if tri < 0:
            steps.append({"decision": MISS, "seg_o": o, "seg_d": d, "list": nlist.meshes()})
            return steps
        before = nlist.meshes()
        s = step(gs, tri, o, d, nlist, k, max_follow, dtype)
        s.update(seg_o=o, seg_d=d, list=before)
        steps.append(s)
        if s["decision"] == GUIDE_HIT:
            return steps
        o, d = s["o"], s["d"]
    raise AssertionError("a chain of max_follow + 1 segments ends on its last hit")
