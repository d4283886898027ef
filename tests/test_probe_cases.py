"""The probe's input grids (probe_cases.py) cannot hide a failure: checked on the CPU through
oracle_eval alone.

 * every range of the libm sources and every outcome class of the shading functions is reached,
   the shading classes by at least 32 cases each (counted from the oracle's outputs and inputs);
 * at most 10 % of an op's cases have a NaN in the oracle's output (the GPU test can only ask for
   "NaN too" there, not for bits);
 * one fixed-seed case per op agrees with a float64 evaluation of the textbook formula to a loose
   relative 1e-4.  That check has one purpose: to catch an op or a field wired to the wrong place
   (the bit-for-bit comparison of device and oracle would not notice a mistake both share).

Counts of this grid (printed with -s): see DESIGN.md, "Probing the device functions".
"""
import math

import numpy as np
import pytest

import probe_cases as pc
from probe_cases import B_DIEL, B_LAMBERT, B_SPECDIEL, B_SPECULAR, B_TS, F32, f32, ubits

MIN_SHADING = 32  # cases per outcome class of a shading op
MIN_LIBM = 1      # every range of a libm source is reached (several hold one value: x == 1, +inf)
NAN_CAP = 0.10


@pytest.fixture(scope="module", autouse=True)
def _oracle(built):
    return True


# ---------------------------------------------------------------- size and NaN share
@pytest.mark.parametrize("op", sorted(pc.GRIDS))
def test_grid_size_and_nan_share(op):
    x, e = pc.grid(op), pc.expected(op)
    assert x.shape == e.shape and x.shape[1] == pc.W and x.dtype == np.float32
    assert 1000 <= len(x) <= 220000, len(x)  # "at most about 2e5": a GPU case stays within seconds
    share = pc.nan_words(op, e).any(axis=1).mean()
    print("%s: %d cases, oracle NaN in %.2f %%" % (op, len(x), 100 * share))
    assert share <= NAN_CAP, share
    # words an op does not define are 0 on the oracle's side (the device must match them too)
    assert not e[:, pc.OUT_WORDS.get(op, 1):].any()
    # deterministic (generated again: the same bits), and the shared copy cannot be written
    assert np.array_equal(ubits(pc.GRIDS[op]()), ubits(x)) and not x.flags.writeable


# ---------------------------------------------------------------- libm ranges
def _count(classes, least):
    for name, m in classes.items():
        print("    %-28s %7d" % (name, int(np.count_nonzero(m))))
    short = {k: int(np.count_nonzero(m)) for k, m in classes.items() if np.count_nonzero(m) < least}
    assert not short, short


def _atanf_id(ix):
    return np.select([ix < 0x3ee00000, ix < 0x3f300000, ix < 0x3f980000, ix < 0x401c0000], [-1, 0, 1, 2], 3)


def test_acosf_ranges():
    hx = ubits(pc.grid("acosf")[:, 0]).astype(np.int64)
    ix, neg = hx & 0x7fffffff, hx >= 0x80000000
    main = (ix < 0x3f800000) & (ix > 0x32800000)
    _count({"x == 1": hx == 0x3f800000, "x == -1": hx == 0xbf800000, "|x| > 1": (ix > 0x3f800000) & (ix <= 0x7f800000),
            "nan": ix > 0x7f800000, "|x| <= 2^-26": ix <= 0x32800000, "|x| < 0.5": main & (ix < 0x3f000000),
            "x <= -0.5": main & (ix >= 0x3f000000) & neg, "x >= 0.5": main & (ix >= 0x3f000000) & ~neg,
            "boundary 0x3f000000": ix == 0x3f000000, "boundary 0x32800000": ix == 0x32800000,
            "boundary 0x32800001": ix == 0x32800001}, MIN_LIBM)


def test_atanf_ranges():
    hx = ubits(pc.grid("atanf")[:, 0]).astype(np.int64)
    ix, neg = hx & 0x7fffffff, hx >= 0x80000000
    main = (ix < 0x4c000000) & (ix >= 0x31000000)
    c = {"nan": ix > 0x7f800000, "x >= 2^25": (ix >= 0x4c000000) & (ix <= 0x7f800000) & ~neg,
         "x <= -2^25": (ix >= 0x4c000000) & (ix <= 0x7f800000) & neg, "|x| < 2^-29": ix < 0x31000000}
    for i in range(-1, 4):
        c["id %d, x > 0" % i] = main & (_atanf_id(ix) == i) & ~neg
        c["id %d, x < 0" % i] = main & (_atanf_id(ix) == i) & neg
    for b in pc.ATAN_CONST:
        c["boundary 0x%08x" % b] = ix == b
        c["below 0x%08x" % b] = ix == b - 1
    _count(c, MIN_LIBM)


def test_atan2f_ranges():
    g = pc.grid("atan2f")
    hy, hx = ubits(g[:, 0]).astype(np.int64), ubits(g[:, 1]).astype(np.int64)
    iy, ix = hy & 0x7fffffff, hx & 0x7fffffff
    nan = (ix > 0x7f800000) | (iy > 0x7f800000)
    one = ~nan & (hx == 0x3f800000)
    m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
    rest = ~nan & ~one
    y0 = rest & (iy == 0)
    x0 = rest & ~y0 & (ix == 0)
    xinf = rest & ~y0 & ~x0 & (ix == 0x7f800000)
    yinf = rest & ~y0 & ~x0 & ~xinf & (iy == 0x7f800000)
    main = rest & ~y0 & ~x0 & ~xinf & ~yinf
    k = (iy - ix) >> 23
    quot = main & ~(k > 60) & ~((hx >= 0x80000000) & (k < -60))
    with np.errstate(all="ignore"):
        qid = _atanf_id(ubits(np.abs(g[:, 0] / g[:, 1])).astype(np.int64))
    c = {"nan": nan, "x == 1": one, "k > 60": main & (k > 60), "x < 0 and k < -60": main & (hx >= 0x80000000) & (k < -60),
         "x > 0 and k < -60": main & (hx < 0x80000000) & (k < -60)}
    for q in range(4):
        c["y == 0, m %d" % q] = y0 & (m == q)
        c["x == 0, m %d" % q] = x0 & (m == q)
        c["x inf, y inf, m %d" % q] = xinf & (iy == 0x7f800000) & (m == q)
        c["x inf, y finite, m %d" % q] = xinf & (iy != 0x7f800000) & (m == q)
        c["y inf, m %d" % q] = yinf & (m == q)
        c["quotient, m %d" % q] = quot & (m == q)
        for kk in (-61, -60, 60, 61):
            c["k == %d, m %d" % (kk, q)] = main & (k == kk) & (m == q)
    for i in range(-1, 4):
        c["quotient in atanf id %d" % i] = quot & (qid == i)
    _count(c, MIN_LIBM)


@pytest.mark.parametrize("op", ["logf", "logf_lds"])
def test_logf_ranges(op):
    ix = ubits(pc.grid(op)[:, 0]).astype(np.int64)
    special = (ix - 0x00800000) % 2 ** 32 >= 0x7f800000 - 0x00800000
    sub = special & (ix * 2 % 2 ** 32 != 0) & (ix < 0x00800000)
    c = {"x == 1": ix == 0x3f800000, "zero": ix * 2 % 2 ** 32 == 0, "+inf": ix == 0x7f800000,
         "negative or nan": special & (ix != 0x7f800000) & (ix * 2 % 2 ** 32 != 0) & ~sub, "subnormal": sub}
    # the normal path: ix of a subnormal as the source renormalises it
    with np.errstate(all="ignore"):
        nx = np.where(sub, ubits(pc.grid(op)[:, 0] * F32(2.0 ** 23)).astype(np.int64) - (23 << 23), ix)
    ok = (~special | sub) & (ix != 0x3f800000)
    tmp = (nx - pc.LOGF_OFF) % 2 ** 32
    i = (tmp >> 19) % 16
    k = np.where(tmp >= 2 ** 31, tmp - 2 ** 32, tmp) >> 23
    for j in range(16):
        c["table entry %d" % j] = ok & (i == j)
        c["first float of entry %d" % j] = ok & (i == j) & ((tmp & 0x7ffff) == 0)
    c.update({"k < 0": ok & (k < 0), "k == 0": ok & (k == 0), "k > 0": ok & (k > 0), "k == -149 .. -127": ok & (k < -126)})
    _count(c, MIN_LIBM)


def test_sincos_ranges():
    x = pc.grid("sincos")[:, 0]
    assert np.abs(x).max() < 120  # glibc_sincosf's domain: no reduce_large on the device
    top = (ubits(x) >> 20) & 0x7ff
    r = x.astype(np.float64) * float.fromhex("0x1.45F306DC9C883p+23")
    n = (r.astype(np.int32).astype(np.int64) + 0x800000) >> 24
    c = {"|x| < 2^-12": top < ((ubits(F32(2.0 ** -12)) >> 20) & 0x7ff), "|x| < pi/4 otherwise": (n == 0) & (top >= 0x398),
         "n < 0": n < 0, "n >= 4": n >= 4}
    for q in range(4):
        c["n & 3 == %d" % q] = (n & 3) == q
    _count(c, MIN_LIBM)


# ---------------------------------------------------------------- shading outcome classes
def _pair_fr(r):
    """Fr of a (wo, wi) record on the transmission half vector, as bxdf_f's B_DIEL branch computes it."""
    wo, wi = r[:, 9:12], r[:, 12:15]
    below = wo[:, 2] < 0
    eo, ei = np.where(below, r[:, 5], r[:, 8]), np.where(below, r[:, 8], r[:, 5])
    with np.errstate(all="ignore"):
        wh = pc.np_normalize(wo * eo[:, None] + wi * ei[:, None])
        wh = np.where((wh[:, 2] < 0)[:, None], wh * F32(-1), wh)
        c = np.abs(pc.np_dot(wh, wo))
    return pc._oracle_eval("fresnel", pc.records(eo, ei, c))[:, 0]


@pytest.mark.parametrize("op", ["bxdf_f", "bxdf_pdf", "bxdf_f_pdf"])
def test_pair_ops_reach_every_class(op):
    r, e = pc.grid(op), pc.expected(op)
    t = pc.rec_type(r)
    wo, wi = r[:, 9:12], r[:, 12:15]
    zz = wo[:, 2] * wi[:, 2]
    same = r[:, 5] == r[:, 8]
    fr = _pair_fr(r)
    c = {}
    for name, ty in (("dielectric", B_DIEL), ("torrance-sparrow", B_TS)):
        m = t == ty
        c[name + ": reflection"] = m & (zz >= 0)
        c[name + ": wo.z * wi.z < 0"] = m & (zz < 0)
        c[name + ": equal etas"] = m & same
        c[name + ": wo.z < 0"] = m & (wo[:, 2] < 0)
        c[name + ": wo.z * wi.z == 0"] = m & (zz == 0)
        c[name + ": wo.z == +-0"] = m & (wo[:, 2] == 0)
        c[name + ": alpha == 0"] = m & (pc.rec_alpha(r) == 0)
        c[name + ": uap with a0 != ap"] = m & (pc.rec_uap(r) == 1) & (r[:, 6] != r[:, 7])
        c[name + ": wi == -wo"] = m & (wi == -wo).all(axis=1)
        c[name + ": a nonzero finite answer"] = m & np.isfinite(e[:, 0]) & (e[:, 0] != 0)
    d = t == B_DIEL
    c["dielectric: transmission with Fr < 1"] = d & (zz < 0) & (fr < 1)
    c["dielectric: Fr >= 1 in transmission"] = d & (zz < 0) & (fr >= 1)
    c["dielectric: transmission, wo.z < 0"] = d & (zz < 0) & (wo[:, 2] < 0) & (fr < 1)
    for ty, name in ((B_LAMBERT, "lambert"), (B_SPECULAR, "specular"), (B_SPECDIEL, "specular dielectric")):
        c[name] = t == ty
    print(op)
    _count(c, MIN_SHADING)


def test_sample_f_reaches_every_class():
    r, e = pc.grid("bxdf_sample_f"), pc.expected("bxdf_sample_f")
    t = pc.rec_type(r)
    wo = r[:, 9:12]
    same = r[:, 5] == r[:, 8]
    fl = ubits(e[:, 7])
    fl_in = (ubits(r[:, 0]) >> 16) & 0xFF
    fr = pc.fresnel_of_wh(r)
    cmpv = np.where(t == B_SPECDIEL, r[:, 13], r[:, 12])  # B_DIEL compares s1, B_SPECDIEL sample.x
    trans = (fl & pc.F_TRANSMISSIVE) != 0
    alpha = pc.rec_alpha(r)
    # sin_i of the (2, 1) critical-angle cases (B_SPECDIEL: of wo.z itself)
    sd = (t == B_SPECDIEL) & ~same
    below = wo[:, 2] < 0
    eo, ei = np.where(below, r[:, 5], r[:, 8]), np.where(below, r[:, 8], r[:, 5])
    with np.errstate(all="ignore"):
        sin_i = (eo / ei) * np.sqrt(F32(1) - wo[:, 2] * wo[:, 2])
    c = {}
    for name, ty in (("dielectric", B_DIEL), ("specular dielectric", B_SPECDIEL)):
        m = (t == ty) & ~same
        c[name + ": reflection (below Fr)"] = m & (cmpv < fr)
        c[name + ": transmission"] = m & trans
        c[name + ": TIR (at or above Fr, not transmissive)"] = m & (cmpv >= fr) & ~trans
        c[name + ": at Fr exactly"] = m & (cmpv == fr)
        c[name + ": just below Fr"] = m & (cmpv == np.nextafter(fr, F32(-np.inf)))
        c[name + ": just above Fr"] = m & (cmpv == np.nextafter(fr, F32(np.inf)))
        c[name + ": equal etas, incoming flags 0"] = (t == ty) & same & (fl_in == 0)
        c[name + ": equal etas, incoming flags all ones"] = (t == ty) & same & (fl_in == 0xFF) & (fl == 0xFF)
        c[name + ": wo.z < 0"] = m & below
        c[name + ": wo.z < 0, transmission"] = m & below & trans
        c[name + ": wo.z * wi.z == 0"] = (t == ty) & (wo[:, 2] * e[:, 5] == 0)
    c["specular dielectric: sin_i == 1"] = sd & (sin_i == 1)
    # (the nearest values 2 sqrt(1 - z * z) can take: probe_cases.critical_wo)
    c["specular dielectric: sin_i just below 1"] = sd & (sin_i < 1) & (sin_i >= F32(1) - F32(2.0 ** -23))
    c["specular dielectric: sin_i just above 1"] = sd & (sin_i > 1) & (sin_i <= F32(1) + F32(2.0 ** -22))
    for name, ty in (("dielectric", B_DIEL), ("torrance-sparrow", B_TS)):
        m = (t == ty) & ~((ty == B_DIEL) & same)
        for bit, fn in ((pc.F_SPECULAR, "specular"), (pc.F_GLOSSY, "glossy"), (pc.F_DIFFUSE, "diffuse")):
            c["%s: flags %s" % (name, fn)] = m & ((fl & 7) == bit)
        thr = F32(1e-4) if ty == B_DIEL else F32(1e-3)
        c[name + ": alpha at its threshold"] = m & (alpha == thr) & ((fl & 7) == pc.F_SPECULAR)
        c[name + ": alpha just above its threshold"] = m & (alpha == np.nextafter(thr, F32(1))) & ((fl & 7) == pc.F_GLOSSY)
        c[name + ": alpha == 1"] = m & (alpha == 1) & ((fl & 7) == pc.F_DIFFUSE)
        c[name + ": uap with a0 != ap"] = m & (pc.rec_uap(r) == 1) & (e[:, 8] == r[:, 7]) & (r[:, 6] != r[:, 7])
        c[name + ": wo == (0, 0, +-1)"] = m & (wo[:, 0] == 0) & (wo[:, 1] == 0)
        c[name + ": wo.z < 0"] = m & below
        c[name + ": wo.z == +-0"] = (t == ty) & (wo[:, 2] == 0)
        c[name + ": a nonzero finite f"] = m & np.isfinite(e[:, 0]) & (e[:, 0] != 0)
    c["lambert"] = t == B_LAMBERT
    c["specular"] = t == B_SPECULAR
    c["specular: wo.z == +-0"] = (t == B_SPECULAR) & (wo[:, 2] == 0)
    print("bxdf_sample_f")
    _count(c, MIN_SHADING)


def test_fresnel_reaches_every_class():
    r, e = pc.grid("fresnel"), pc.expected("fresnel")
    eo, ei, cth = r[:, 0], r[:, 1], r[:, 2]
    with np.errstate(all="ignore"):
        co = np.minimum(np.abs(cth), F32(1))
        sin_i = (eo / ei) * np.sqrt(F32(1) - co * co)
    ne = eo != ei
    print("fresnel")
    _count({"equal etas": eo == ei, "sin_i > 1": ne & (sin_i > 1), "sin_i == 1": ne & (sin_i == 1),
            "sin_i just below 1": ne & (sin_i < 1) & (sin_i >= F32(1) - F32(2.0 ** -23)),
            "sin_i just above 1": ne & (sin_i > 1) & (sin_i <= F32(1) + F32(2.0 ** -22)), "|cos| > 1 (clamped)": ne & (np.abs(cth) > 1),
            "cos < 0": ne & (cth < 0), "cos == +-0": ne & (cth == 0), "between 0 and 1": ne & (e[:, 0] > 0) & (e[:, 0] < 1)},
           MIN_SHADING)


def test_sampling_grids_hold_the_edges():
    for op in ("uniform_sample_disk", "uniform_sample_ring", "cosine_sample_hemisphere", "uniform_sample_sphere", "sample_wh"):
        r = pc.grid(op)
        for a in pc.SAMPLE_EDGES:
            for b in pc.SAMPLE_EDGES:
                assert ((r[:, 0] == a) & (r[:, 1] == b)).any(), (op, a, b)
        assert r[:, :2].min() >= 0 and r[:, :2].max() < 1
    r = pc.grid("uniform_sample_ring")
    for i in pc.INNER:
        assert np.count_nonzero(r[:, 2] == i) >= 25
    r = pc.grid("rng_int")
    for m in pc.RNG_MAX:
        for s in (0, 1, 0xFFFFFFFF):
            assert ((ubits(r[:, 0]) == s) & (ubits(r[:, 1]) == m)).any(), (s, m)


# ---------------------------------------------------------------- textbook values (wiring only)
def _one(op, *words):
    x = np.zeros((1, pc.W), np.float32)
    for k, w in enumerate(words):
        x[0, k] = np.uint32(w).view(np.float32) if isinstance(w, (int, np.integer)) else F32(w)
    return x, pc._oracle_eval(op, x)[0]


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.abs(got - want) <= 1e-4 * np.abs(want) + 1e-30), (got, want)


def _xorshift(y):
    y ^= (y << 13) & 0xFFFFFFFF
    y ^= y >> 17
    y ^= (y << 5) & 0xFFFFFFFF
    return y


def _ggx_d(a, wh):
    c2 = wh[2] ** 2
    t2 = (1 - c2) / c2
    return a * a / (math.pi * c2 * c2 * (a * a + t2) ** 2)


def _smith_lambda(a, w):
    t2 = (1 - w[2] ** 2) / w[2] ** 2
    return (-1 + math.sqrt(1 + a * a * t2)) / 2


def _fresnel64(eo, ei, c):
    c = min(abs(c), 1.0)
    st = eo / ei * math.sqrt(1 - c * c)
    if st > 1:
        return 1.0
    ct = math.sqrt(1 - st * st)
    rp = (ei * c - eo * ct) / (ei * c + eo * ct)
    rs = (eo * c - ei * ct) / (eo * c + ei * ct)
    return (rp * rp + rs * rs) / 2


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _vndf64(wo, a, s, diel):
    """Visible-normal sampling of GGX in the reference's frame convention (T1 = (h.y, -h.x, 0), the
    disk's x on T1 and its warped y on T2), float64."""
    h = _unit([wo[0] * a, wo[1] * a, wo[2]])
    if diel and wo[2] < 0:
        h = -h
    t1 = np.array([1.0, 0, 0]) if (diel and wo[0] == 0 and wo[1] == 0) else _unit([h[1], -h[0], 0])
    t2 = _unit(np.cross(t1, h))
    r, th = math.sqrt(s[0]), 2 * math.pi * s[1]
    vx, vy = r * math.cos(th), r * math.sin(th)
    k = (1 + h[2]) / 2
    vy = k * vy + (1 - k) * math.sqrt(1 - vx * vx)
    w = h * math.sqrt(max(0.0, 1 - vx * vx - vy * vy)) + t1 * vx + t2 * vy
    return _unit([w[0] * a, w[1] * a, w[2]])


def _ts_f_pdf64(rho, a, eta_outer, eta, wo, wi):
    wh = _unit(wo + wi)
    d, g1 = _ggx_d(a, wh), 1 / (1 + _smith_lambda(a, wo))
    g = 1 / (1 + _smith_lambda(a, wo) + _smith_lambda(a, wi))
    f = np.asarray(rho, np.float64) * g * d * _fresnel64(eta_outer, eta, float(wh @ wi)) / (4 * wo[2] * wi[2])
    return f, d * g1 / (4 * wo[2])


def _shade_case(typ, wo, c12, c13, c14, a0=0.2, ap=0.35, uap=0, eta=1.5, eta_outer=1.0):
    return pc.shade_records(typ, uap, 0, pc.RHO, pc.TAU, f32([eta]), f32([ap if uap else a0]), f32([eta_outer]),
                            f32([wo]), F32(c12), F32(c13), F32(c14)), (ap if uap else a0)


def test_one_case_per_op_matches_the_textbook():
    rng = np.random.default_rng(20240607)
    u = lambda lo, hi: float(F32(rng.uniform(lo, hi)))  # noqa: E731
    v = u(-0.9, 0.9)
    _close(_one("acosf", v)[1][0], math.acos(v))
    v = u(1, 5)
    _close(_one("atanf", v)[1][0], math.atan(v))
    y, x = u(0.5, 2), u(-3, -1)
    _close(_one("atan2f", y, x)[1][0], math.atan2(y, x))
    v = u(0.1, 0.9)
    _close(_one("logf", v)[1][0], math.log(v))
    _close(_one("logf_lds", v)[1][0], math.log(v))
    v = u(0.5, 6)
    _close(_one("sincos", v)[1][:2], [math.sin(v), math.cos(v)])
    v = u(1000, 5000)
    assert ubits(_one("f2u32", v)[1][0]) == int(v)
    assert ubits(_one("f2u8", v)[1][0]) == int(v) % 256
    a, b = u(-20, -5), 2 * math.pi
    _close(_one("gmod", a, b)[1][0], a - float(F32(b)) * math.floor(a / float(F32(b))))
    v = u(-9, -1)
    _close(_one("gfract", v)[1][0], v - math.floor(v))
    st, mx = int(rng.integers(1, 2 ** 32)), int(rng.integers(2, 1000))
    o = _one("rng_float", st)[1]
    nxt = _xorshift(st)
    _close(o[0], ((nxt * 0x9E3779BB) & 0xFFFFFFFF) / 2.0 ** 32)
    assert ubits(o[1]) == nxt
    o = _one("rng_int", st, mx)[1]
    assert ubits(o[0]) == (((nxt * 0x9E3779B9) & 0xFFFFFFFF) * (mx + 1)) >> 32 and ubits(o[1]) == nxt
    sx, sy, inner = u(0.1, 0.9), u(0.05, 0.95), u(0.2, 0.8)
    th = 2 * math.pi * sy
    _close(_one("uniform_sample_disk", sx, sy)[1][:2], [math.sqrt(sx) * math.cos(th), math.sqrt(sx) * math.sin(th)])
    rr = math.sqrt(inner * (1 - sx) + sx)
    _close(_one("uniform_sample_ring", sx, sy, inner)[1][:3], [rr * math.cos(th), rr * math.sin(th), 1 / (math.pi * (1 - inner))])
    z = math.sqrt(1 - sx)
    _close(_one("cosine_sample_hemisphere", sx, sy)[1][:4], [math.sqrt(sx) * math.cos(th), math.sqrt(sx) * math.sin(th), z, z / math.pi])
    z = 1 - 2 * sx
    _close(_one("uniform_sample_sphere", sx, sy)[1][:3], [math.sqrt(1 - z * z) * math.cos(th), math.sqrt(1 - z * z) * math.sin(th), z])
    wo = _unit([u(0.2, 0.6), u(-0.6, -0.2), u(0.5, 0.9)]).astype(np.float32)
    alpha = u(0.1, 0.6)
    for diel in (0, 1):
        x = np.zeros((1, pc.W), np.float32)
        x[0, :3] = sx, sy, alpha
        x[0, 3] = np.uint32(diel).view(np.float32)
        x[0, 4:7] = wo * (F32(-1) if diel else F32(1))
        _close(pc._oracle_eval("sample_wh", x)[0, :3], _vndf64(x[0, 4:7].astype(np.float64), alpha, (sx, sy), diel))
    c = u(0.3, 0.9)
    _close(_one("fresnel", 1.0, 1.5, c)[1][0], _fresnel64(1.0, 1.5, c))
    # Torrance-Sparrow, both above the surface; uap picks alpha_prime
    wi = _unit([u(-0.5, 0.5), u(-0.5, 0.5), u(0.4, 0.9)]).astype(np.float32)
    x, al = _shade_case(B_TS, wo, wi[0], wi[1], wi[2], uap=1)
    f64, p64 = _ts_f_pdf64(pc.RHO, al, 1.0, 1.5, wo.astype(np.float64), wi.astype(np.float64))
    _close(pc._oracle_eval("bxdf_f", x)[0, :3], f64)
    _close(pc._oracle_eval("bxdf_pdf", x)[0, 0], p64)
    # the dielectric in transmission (Walter et al. 2007, eq. 21 and 17): wi below the surface
    wt = _unit([-wo[0] * 0.5, -wo[1] * 0.5, -0.8]).astype(np.float32)
    x, al = _shade_case(B_DIEL, wo, wt[0], wt[1], wt[2])
    o, i = wo.astype(np.float64), wt.astype(np.float64)
    eo, ei = 1.0, 1.5
    wh = _unit(o * eo + i * ei)
    wh = -wh if wh[2] < 0 else wh
    d, lo, li = _ggx_d(al, wh), _smith_lambda(al, o), _smith_lambda(al, i)
    fr = _fresnel64(eo, ei, float(wh @ o))
    den = (ei * (i @ wh) + eo * (o @ wh)) ** 2
    ft = abs(i @ wh) * abs(o @ wh) * eo * eo * (1 - fr) * d / (1 + lo + li) / (den * abs(o[2] * i[2]))
    pt = d * abs(o @ wh) / (1 + lo) / abs(o[2]) * abs(i @ wh) * ei * ei / den
    tau = float(pc.TAU)
    got = pc._oracle_eval("bxdf_f_pdf", x)[0]
    assert ft > 1e-6 and pt > 1e-6
    _close(got[:4], [ft * tau, ft * tau / 2, ft * tau / 4, pt])
    # bxdf_sample_f, Torrance-Sparrow: wi mirrors wo about the sampled wh; f and pdf are those of (wo, wi)
    x, al = _shade_case(B_TS, wo, 0.5, sx, sy)
    got = pc._oracle_eval("bxdf_sample_f", x)[0]
    wh = _vndf64(wo.astype(np.float64), al, (sx, sy), 0)
    wi64 = _unit(2 * (wo.astype(np.float64) @ wh) * wh - wo)
    f64, p64 = _ts_f_pdf64(pc.RHO, al, 1.0, 1.5, wo.astype(np.float64), wi64)
    _close(got[3:6], wi64)
    _close(got[:3], f64)
    _close(got[6], p64)
    assert ubits(got[7]) == pc.F_GLOSSY and got[8] == F32(al)
