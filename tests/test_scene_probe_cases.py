"""The record sets of the device scene probe (scene_probe_cases.py) reach what they are designed for: CPU,
oracle.scene_eval alone.

Every class holds at least 32 records in every scene that can produce it (the floor of the shading grids,
DESIGN.md), and where the oracle's answer can show that a class took its branch -- a zero row that leaves pdf
alone, a roughness on either side of a threshold, a rim that is hit at r2 and missed just beyond -- it is asked.
At most 10 % of an op's records have an oracle NaN in a compared word (the GPU test can only ask for "NaN
too" there), the records that read outside a reference table are exactly the ones never sent to the device,
no record is set aside, and one record per op agrees with a float64 textbook evaluation (wiring only).
"""
import numpy as np
import pytest

import nart_amd
import oracle
import scene_probe_cases as sp

f32 = np.float32
EPS = 2.0 ** -24  # half an ulp of a float32 in [1, 2): the relative error bound of one rounded operation
FLOOR = 32


@pytest.fixture(scope="module")
def scene_dir(built, tmp_path_factory):
    return str(tmp_path_factory.mktemp("scene_probe"))


def _ops(name, scene_dir):
    return sp.prepared(name, scene_dir)["ops"]


@pytest.mark.parametrize("name", sp.SCENES)
def test_every_class_is_populated(scene_dir, name):
    for op, p in _ops(name, scene_dir).items():
        assert 6000 <= len(p["x"]) <= 80000, (op, len(p["x"]))
        for c in p["classes"]:
            n = int(sp.of_class(p, c).sum())
            print("%s %s %s: %d" % (name, op, c, n))
            assert n >= FLOOR, (name, op, c, n)


def test_scenes_produce_the_classes_they_are_for(scene_dir):
    """Which scene can produce which class is stated here, not left to whatever the generators emit."""
    has = lambda name, op, c: c in _ops(name, scene_dir)[op]["classes"]  # noqa: E731
    for c in ("r2_at", "r2_below", "r2_above", "ri2_at", "ri2_below", "ri2_above", "grazing", "grazing_front", "grazing_back",
              "t_near_zero", "on_plane", "at_centre", "unnormalised", "pole", "phi_pi", "phi_zero", "beyond_unit"):
        assert has("lights", "light_li", c), c
    for c in ("sample_edges", "behind", "on_plane", "at_centre", "row_border"):
        assert has("lights", "light_sample_li", c), c
    assert has("env_zero_rows", "light_sample_li", "zero_row_aim") and has("env_one_texel_row", "light_sample_li", "one_texel_row")
    for name in ("materials", "mat_envtex"):
        for c in ("threshold", "normal_zero", "normal_minus_z", "normal_tangent", "dpds_parallel"):
            assert has(name, "create_bsdf", c), (name, c)
    assert has("mat_glass", "create_bsdf", "threshold") and has("mat_diffuse", "create_bsdf", "dpds_parallel")
    for name in sp.MEDIA:
        for c in ("zero", "clamp_high", "below_zero", "above_one", "lattice_plane"):
            assert has(name, "dg_lookup", c), (name, c)
        for c in ("inside", "outside_toward", "pointing_away", "on_face", "on_edge", "at_corner", "zero_component", "grazing",
                  "unnormalised"):
            assert has(name, "medium_walk", c), (name, c)
    for t in sp.ENV_TEXTURES:
        for op, c in (("tex_fetch", "clamp_low"), ("tex_fetch", "clamp_high"), ("tex_fetch", "flip"), ("tex_fetch", "texel_border"),
                      ("env_pdf", "clamp"), ("env_pdf", "cell_border"), ("env_pdf", "below_zero")):
            assert has("env_" + t, op, c), (t, op, c)


def test_area_light_rims_are_hit_and_missed_where_designed(scene_dir):
    """dist == r2 is a hit and the next float a miss (dist > r2 returns 0); dist == ri2 is a hit and the float
    below a miss.  A miss leaves the preset pdf; shown on the records that ask for the pdf with the sentinel."""
    for name in ("lights", "mat_diffuse", "mat_glass", "materials"):
        p = _ops(name, scene_dir)["light_li"]
        asks = (p["x"][:, 7].view(np.uint32) != 0) & (p["x"][:, 9] == sp.SENTINEL)
        hit = p["want"][:, 3] != sp.SENTINEL
        for c, want_hit in (("r2_below", True), ("r2_at", True), ("r2_above", False)) + \
                ((("ri2_below", False), ("ri2_at", True), ("ri2_above", True)) if name == "lights" else ()):
            m = sp.of_class(p, c) & asks
            assert m.sum() >= 8 and np.all(hit[m] == want_hit), (name, c, int(m.sum()), int(hit[m].sum()))
    p = _ops("lights", scene_dir)["light_li"]
    asks = (p["x"][:, 7].view(np.uint32) != 0) & (p["x"][:, 9] == sp.SENTINEL)
    hit = p["want"][:, 3] != sp.SENTINEL
    # dot(wi, n) of exactly +-0 and of either sign next to it, by area_pdf's own float32 dot product
    lights = sp.prepared("lights", scene_dir)["scene"].lights()
    li = p["x"][:, 0].view(np.uint32)
    dn = np.full(len(li), np.nan, f32)
    for k in np.unique(li[li < 24]):
        m = li == k
        dn[m] = sp.area_terms(lights[k], p["x"][m, 1:4], p["x"][m, 4:7])[0]
    zero, front, back = sp.of_class(p, "grazing") & (dn == 0), sp.of_class(p, "grazing_front") & (dn < 0), sp.of_class(p, "grazing_back") & (dn > 0)
    print("dot(wi, n): +0 %d, -0 %d, below 0 %d, above 0 %d" % ((zero & ~np.signbit(dn)).sum(), (zero & np.signbit(dn)).sum(), front.sum(), back.sum()))
    assert (zero & ~np.signbit(dn)).sum() >= FLOOR and (zero & np.signbit(dn)).sum() >= FLOOR and front.sum() >= FLOOR and back.sum() >= FLOOR
    assert not hit[(zero | back) & asks].any()  # dot(wi, n) >= 0 returns 0
    assert (sp.of_class(p, "t_near_zero") & asks & hit).sum() >= FLOOR and (sp.of_class(p, "t_near_zero") & asks & ~hit).sum() >= FLOOR


def test_zero_rows_and_the_single_texel_row_are_sampled(scene_dir):
    """A sample that lands in a row of zero texels leaves pdf alone (texturepattern.cpp:99 is a no-op): with the
    sentinel preset the answer's pdf is negative, which no other path produces.  Samples aimed at the row with
    one bright texel return that texel's direction: one phi for the whole class."""
    p = _ops("env_zero_rows", scene_dir)["light_sample_li"]
    left_alone = (p["x"][:, 9] == sp.SENTINEL) & (p["want"][:, 3] < 0)
    print("zero-row records:", int(left_alone.sum()), "of them aimed:", int((left_alone & sp.of_class(p, "zero_row_aim")).sum()))
    assert left_alone.sum() >= FLOOR
    for name in ("env_sky", "env_equal_row", "env_1x1"):  # strictly positive maps never take it
        q = _ops(name, scene_dir)["light_sample_li"]
        assert not ((q["x"][:, 9] == sp.SENTINEL) & (q["want"][:, 3] < 0)).any()
    p = _ops("env_one_texel_row", scene_dir)["light_sample_li"]
    m = sp.of_class(p, "one_texel_row") & sp.sendable(p)
    wi = p["want"][m, 5:8]
    phi = np.arctan2(wi[:, 1], wi[:, 0])
    assert m.sum() >= FLOOR and np.ptp(np.unwrap(phi)) < 2 * np.pi / 12  # inside the one texel's column


def test_roughness_lands_on_either_side_of_the_thresholds(scene_dir):
    """The threshold class: ap = 1 - (1 - alpha) * alphaTweak on the two values it can take nearest to 1e-4
    (1e-3 for plastic) and a few steps out, from constant and textured alpha: both outcomes, glossy with that ap
    and specular, in every kind that has the threshold."""
    for name, kinds in (("materials", (1, 2, 3, 4)), ("mat_envtex", (4,)), ("mat_glass", (2,))):
        p = _ops(name, scene_dir)["create_bsdf"]
        mats = sp.prepared(name, scene_dir)["scene"].materials()
        kind = np.array([mats[i].type for i in p["x"][:, 0].view(np.uint32)])
        th = sp.of_class(p, "threshold")
        for k in kinds:
            lobe = 21 if k == nart_amd.api.MAT_PLASTIC else 10
            thr = sp.THRESHOLDS[1] if k == nart_amd.api.MAT_PLASTIC else sp.THRESHOLDS[0]
            m = th & (kind == k)
            t = p["want"][m, lobe].view(np.uint32)
            ap = p["want"][m, lobe + 10]
            rough, spec = (t == sp.B_TS) | (t == sp.B_DIEL), (t == sp.B_SPECULAR) | (t == sp.B_SPECDIEL)
            print(name, "kind", k, "threshold records", int(m.sum()), "glossy", int(rough.sum()), "specular", int(spec.sum()))
            assert np.all(rough | spec) and rough.sum() >= 8 and spec.sum() >= 8, (name, k, int(rough.sum()), int(spec.sum()))
            k0 = np.floor(float(thr) * 2 ** 24)
            assert np.any(ap[rough] == f32((k0 + 1) * 2.0 ** -24)) and np.all(ap[rough] > thr), (name, k)


def test_normal_map_texels_decode_as_designed(scene_dir):
    p = _ops("materials", scene_dir)["create_bsdf"]
    n = p["want"][:, 0:3]
    assert np.isnan(n[sp.of_class(p, "normal_zero")]).all()
    sn = p["x"][:, 3:6]
    mz = sp.of_class(p, "normal_minus_z")
    assert np.allclose(n[mz], -sn[mz], atol=1e-5)  # to_world of (0, 0, -1): the flipped shading normal
    par = sp.of_class(p, "dpds_parallel")
    assert np.isnan(p["want"][par, 3:6]).any(axis=1).mean() > 0.25  # n_t = normalize(0) where dpds || n exactly


def test_medium_walks_reach_both_answers_and_several_segments(scene_dir):
    for name in sp.MEDIA:
        p = _ops(name, scene_dir)["medium_walk"]
        ok = p["want"][:, 0].view(np.uint32)
        ns = p["want"][:, 1].view(np.uint32)
        used = p["want"][:, 7::4].view(np.uint32)
        print(name, "hit", int((ok == 1).sum()), "miss", int((ok == 0).sum()), "segments", np.bincount(ns, minlength=8).tolist(),
              "largest majorant index", int(used.max()))
        assert (ok == 1).sum() >= FLOOR and (ok == 0).sum() >= FLOOR and (ns[ok == 1] == 0).sum() >= FLOOR
        assert (ns >= 1).sum() >= FLOOR and ns.max() <= nart_amd.SCENE_WALK_SEGMENTS and used.max() < 7
        if name != "med_255_tiny":  # its chords are shorter than the iterator's 1e-4 step: none or the cap
            assert (ns == 1).sum() >= FLOOR and (ns >= 2).sum() >= FLOOR
        touch = (ok == 1) & (p["want"][:, 2] == p["want"][:, 3])
        print(name, "tMin == tMax:", int(touch.sum()))


@pytest.mark.parametrize("name", sp.SCENES)
def test_nan_share_oob_and_set_aside(scene_dir, name):
    for op, p in _ops(name, scene_dir).items():
        send = sp.sendable(p)
        assert np.array_equal(send, (p["flags"] & oracle.SCENE_OOB) == 0)
        share, aside = sp.nan_share(op, p), float(sp.set_aside(op, p).mean())
        print("%s %s: %d records, %d off a table, NaN %.2f %%, set aside %.2f %%" % (name, op, len(p["x"]), int((~send).sum()), 100 * share, 100 * aside))
        assert share <= 0.10, (name, op, share)
        assert aside < 0.01 and send.mean() > 0.9, (name, op, aside, send.mean())
        if "nan_coordinate" in p["classes"]:
            assert not send[sp.of_class(p, "nan_coordinate")].any()  # (int)NaN is INT_MIN on x86: off the texture
        if "off_table" in p["classes"]:
            assert (~send[sp.of_class(p, "off_table")]).sum() >= FLOOR  # a coordinate a cell or more below 0


def test_oracle_validates_its_arguments(scene_dir):
    prep = sp.prepared("lights", scene_dir)
    lib, h = oracle.lib(), prep["oracle"]._h
    x = sp.records(2)
    y = np.full((2, nart_amd.SCENE_OUT_WORDS), 5.0, f32)
    fl = np.zeros(2, np.uint32)
    call = lambda op, xi=x: lib.oracle_scene_eval(h, op, xi.ctypes.data, 2, y.ctypes.data, fl.ctypes.data)  # noqa: E731
    assert call(len(nart_amd.SCENE_OPS)) == -1
    assert call(nart_amd.SCENE_OPS["dg_lookup"]) == -1 and call(nart_amd.SCENE_OPS["medium_walk"]) == -1  # no medium
    bad = x.copy()
    for op, count in (("tex_fetch", 2), ("light_li", 27), ("create_bsdf", 1)):
        bad[1, 0] = np.uint32(count).view(f32)
        assert call(nart_amd.SCENE_OPS[op], bad) == -1, op
    assert call(nart_amd.SCENE_OPS["env_pdf"]) == -1  # light 0 is a disk
    assert lib.oracle_scene_eval(h, 0, None, 2, y.ctypes.data, fl.ctypes.data) == -1 and np.all(y == 5.0)


# ------------------------------------------------------------------------------------------------ wiring
def _one(name, scene_dir, op, x):
    out, flags = oracle.scene_eval(sp.prepared(name, scene_dir)["oracle"], op, x)
    assert flags[0] == 0
    return out[0]


def _close(got, want, ops, scale=None):
    """|got - want| <= ops * 2^-24 * scale: `ops` rounded float32 operations on the way, each within half an ulp
    of a value no larger than scale (default: the value itself)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = ops * EPS * (np.abs(want) if scale is None else scale)
    assert np.all(np.abs(got - want) <= tol), (got, want, tol)


def test_wiring_against_float64(scene_dir):
    """One record per op against a float64 evaluation of what the function is meant to compute.  Each tolerance
    is the count of float32 operations between the inputs and the word, times 2^-24 of the largest intermediate."""
    # tex_fetch: a texel centre returns the texel (no arithmetic); squared with the roughness flag (1 operation)
    sc = sp.prepared("env_zero_rows", scene_dir)["scene"]
    tex = sc.textures()[0].view(np.float16).astype(np.float64)
    x = sp.records(1)
    x[0, 1], x[0, 2] = (5 + 0.5) / 37, 1 - (3 + 0.5) / 19
    _close(_one("env_zero_rows", scene_dir, "tex_fetch", x)[:3], tex[3, 5, :3], 0)
    x[0, 3] = sp.u32(1)
    _close(_one("env_zero_rows", scene_dir, "tex_fetch", x)[:3], tex[3, 5, :3] ** 2, 1)
    # env_pdf: texel luminance over the map's mean luminance.  Row sums of 37 texels of 3 channels (111 additions),
    # 19 row sums, two normalisations and the product: 140 operations
    lum = np.abs(tex[..., :3]).sum(-1)
    x = sp.records(1)
    x[0, 1], x[0, 2] = (5 + 0.5) / 37, 1 - (3 + 0.5) / 19
    _close(_one("env_zero_rows", scene_dir, "env_pdf", x)[0], lum[3, 5] / lum.mean(), 140)
    # light_li / light_bound: light 1 of "lights" is the identity disk of radius 1 facing -z; from (0.2, 0.1, -2)
    # along +z the hit is at t = 2 (exact in float32), pdf = t^2 / (pi r^2 cos) = 4 / pi: 1/(pi r r) 3 operations,
    # t*t, the division and the product: 6; Li = Le * intensity: 1
    L = sp.prepared("lights", scene_dir)["scene"].lights()[1]
    assert L.type == nart_amd.api.LIGHT_DISK and L.radius == 1.0
    x = sp._li_rec(1, [(0.2, 0.1, -2.0)], [(0.0, 0.0, 1.0)])
    got = _one("lights", scene_dir, "light_li", x)
    _close(got[:3], np.array(L.Le.value[:], np.float64) * L.intensity, 1)
    _close(got[3], 4 / np.pi, 6)
    assert got[4] == 2.0 and _one("lights", scene_dir, "light_bound", x)[4] == 2.0
    # light_sample_li: whatever point the sample maps to, it lies on the disk, wi points at it from p, tMax is its
    # distance and pdf = dist^2 / (pi r^2 cos).  The point: 2 products and the matrix row (7); wi, dist: 3
    # subtractions, the squared length (5), sqrt, the normalisation (5): 20 in all, and 8 more for the pdf
    x = sp.records(1)
    x[0, 0], x[0, 1:4], x[0, 4:6] = sp.u32(1), (0.3, -0.2, -1.5), (0.3, 0.8)
    got = _one("lights", scene_dir, "light_sample_li", x).astype(np.float64)
    p, wi, dist = np.array([0.3, -0.2, -1.5]), got[5:8], got[4]
    hit = p + wi * dist
    _close(np.linalg.norm(wi), 1.0, 20)
    _close(hit[2], 0.0, 20, scale=2.0)
    assert hit[0] ** 2 + hit[1] ** 2 <= 1.0 + 40 * EPS
    _close(got[3], dist ** 2 / (np.pi * wi[2]), 28)
    # create_bsdf: material 0 of "materials" is a constant Lambert; sn = z, dpds = x gives the frame (x, y, z):
    # exact products with 0 and 1, normalisations of unit vectors (sqrt(1) = 1): 0 operations that round
    m = sp.prepared("materials", scene_dir)["scene"].materials()[0]
    x = sp.records(1)
    x[0, 3:6], x[0, 6:9], x[0, 9] = (0, 0, 1), (1, 0, 0), 0.5
    got = _one("materials", scene_dir, "create_bsdf", x)
    _close(got[:9], [0, 0, 1, 1, 0, 0, 0, 1, 0], 0, scale=1.0)
    assert got[9:12].view(np.uint32).tolist() == [1, sp.B_LAMBERT, 4] and np.array_equal(got[12:15], f32(m.rho_d.value[:]))
    assert not got[15:].any()
    # dg_lookup: trilinear interpolation on the 4x3x5 grid.  Per axis a clamp-scale product and a subtraction (2),
    # seven mixes of 4 operations each: 34 operations on values no larger than the largest density
    med = sp.prepared("med_435_none", scene_dir)["scene"].medium()
    d = med["density"].astype(np.float64)
    q = np.array([0.3, 0.6, 0.2])

    def trilinear(q):
        g = np.clip(q, 0, 0.999) * (np.array(med["res"]) - 1)
        i0 = np.floor(g).astype(int)
        fr = g - i0
        v = 0.0
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w = (fr[0] if dx else 1 - fr[0]) * (fr[1] if dy else 1 - fr[1]) * (fr[2] if dz else 1 - fr[2])
                    v += w * d[i0[2] + dz, i0[1] + dy, i0[0] + dx]
        return v

    want = trilinear(q)
    x = sp.records(1)
    x[0, :3] = q
    got = _one("med_435_none", scene_dir, "dg_lookup", x)
    _close(got[0], want, 34, scale=d.max())
    assert got[1] == got[0] and got[2] == 0 and got[3].view(np.uint32) == 0
    # medium_walk: from outside along +x through the box's middle: enters at bmin.x, leaves at bmax.x, one
    # majorant segment over the whole chord with sigma = majorant * (sigma_a + sigma_s), the majorant being the
    # largest of the grid points short of each axis' last one (media.cpp:47-130 stops there) and of the eight
    # corner look-ups: 34 operations, the sum and the product.  Slab distances: a
    # subtraction and a division each (2); the segment end adds the crossing distance, itself a division, two
    # products and the entry's own rounding: 8, on values up to the exit distance
    lo, hi = med["bounds_min"].astype(np.float64), med["bounds_max"].astype(np.float64)
    o = np.array([lo[0] - 1.5, (lo[1] + hi[1]) / 2, (lo[2] + hi[2]) / 2])
    x = sp.records(1)
    x[0, :3], x[0, 3:6] = o, (1, 0, 0)
    got = _one("med_435_none", scene_dir, "medium_walk", x)
    assert got[:2].view(np.uint32).tolist() == [1, 1] and got[7].view(np.uint32) == 0
    _close(got[2], 1.5, 2)
    _close(got[3], 1.5 + hi[0] - lo[0], 2)
    majorant = max([d[:-1, :-1, :-1].max()] + [trilinear(np.array([cx, cy, cz], float)) for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)])
    _close(got[4], majorant * (med["sigma_a"] + med["sigma_s"]), 36)
    _close(got[5], 1.5, 2)
    _close(got[6], 1.5 + hi[0] - lo[0], 8)
