"""Input grids of the device probe (nart_hip_eval / oracle_eval): deterministic, no GPU.

grid(op) returns the (n, 16) float32 input records of one op (include/nart_hip.h documents the
fields): designed edges first, then a seeded random fill, at most about 2e5 records.  The CPU test
(test_probe_cases.py) checks through the oracle that the grids reach what they are meant to reach;
the GPU test (test_gpu_probe.py) runs the same records through the device.  The grids need the
oracle only where an input depends on a computed value (s1 at a case's own Fresnel term).
"""
import functools

import numpy as np

W = 16
F32 = np.float32
B_LAMBERT, B_SPECULAR, B_SPECDIEL, B_DIEL, B_TS = range(5)
F_SPECULAR, F_GLOSSY, F_DIFFUSE, F_TRANSMISSIVE = 1, 2, 4, 8
ONE_M = F32(1) - F32(2.0 ** -24)  # the largest float below 1


def f32(x):
    return np.asarray(x, dtype=np.float32)


def bits(u):
    """uint32 bit patterns as float32."""
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def ubits(f):
    return np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)


def around(u, k=1):
    """The bit patterns u - k .. u + k of every pattern in u (its float neighbours)."""
    u = np.atleast_1d(np.asarray(u, dtype=np.int64))
    return ((u[:, None] + np.arange(-k, k + 1)[None, :]).ravel() & 0xFFFFFFFF).astype(np.uint32)


def both_signs(u):
    u = np.asarray(u, dtype=np.uint32)
    return np.concatenate([u, u | np.uint32(0x80000000)])


def records(*cols):
    """Records whose first words are the given equally long columns (float32, or uint32 as bits)."""
    n = len(cols[0])
    r = np.zeros((n, W), np.float32)
    for k, c in enumerate(cols):
        c = np.asarray(c)
        r[:, k] = c.view(np.float32) if c.dtype == np.uint32 else c.astype(np.float32)
    return r


def cross(*axes):
    """Every combination of the rows of the given arrays, as one array per axis."""
    axes = [np.asarray(a) for a in axes]
    idx = np.meshgrid(*[np.arange(len(a)) for a in axes], indexing="ij")
    return [a[i.ravel()] for a, i in zip(axes, idx)]


SPECIAL = np.uint32([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x7f800000, 0xff800000, 0x7fc00000,
                     0xffc00000, 0x7f800001, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000,
                     0x80800000, 0x00800001, 0x7f7fffff, 0xff7fffff])


# ---------------------------------------------------------------- libm
# boundary constants of dmath.h, by function
ACOS_CONST = [0x3f800000, 0x3f000000, 0x32800000]
ATAN_CONST = [0x4c000000, 0x7f800000, 0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000]
LOGF_OFF = 0x3f330000


def grid_acosf():
    u = np.concatenate([SPECIAL, both_signs(around(ACOS_CONST, 2)), both_signs(np.uint32([0x3f800001, 0x3f800002, 0x40000000])),
                        both_signs(np.arange(0, 0x3f800001, 12007, dtype=np.uint32)),
                        np.arange(0x3f800000, 0x7f800000, 30000017, dtype=np.uint32)])
    return records(u.astype(np.uint32))


def grid_atanf():
    u = np.concatenate([SPECIAL, both_signs(around(ATAN_CONST, 2)),
                        np.arange(0, 0x7f800001, 21001, dtype=np.uint32),
                        np.arange(0, 0x7f800001, 42013, dtype=np.uint32) | np.uint32(0x80000000)])
    return records(u.astype(np.uint32))


def grid_atan2f():
    rng = np.random.default_rng(1202)
    parts = []
    # zeros, ones, infinities, NaN, subnormals, ordinary values: every pair, so every quadrant m with
    # every special on either side
    e = np.concatenate([SPECIAL, both_signs(np.uint32([0x40000000, 0x3f000000, 0x0da24260, 0x7149f2ca, 0x3fc00000, 0x40490fdb]))])
    y, x = cross(e, e)
    parts.append(records(y, x))
    # the exponent difference k = (iy - ix) >> 23 at +-60 and +-61 and next to them, every quadrant
    for k in (-62, -61, -60, -59, 59, 60, 61, 62):
        for ex in (64, 127, 127 + 30):
            ey = ex + k
            if not (1 <= ey <= 254):
                ey, ex2 = (254, 254 - k) if ey > 254 else (1, 1 - k)
            else:
                ex2 = ex
            for my, mx in ((0, 0), (0x7fffff, 0), (0, 0x7fffff), (0x123456, 0x654321), (0x654321, 0x123456)):
                yy = np.uint32((ey << 23) | my)
                xx = np.uint32((ex2 << 23) | mx)
                for sy in (0, 0x80000000):
                    for sx in (0, 0x80000000):
                        parts.append(records(np.uint32([yy | sy]), np.uint32([xx | sx])))
    # x == 1: the atanf shortcut, over atanf's own boundaries
    ya = both_signs(around(ATAN_CONST, 1))
    parts.append(records(ya, np.full(len(ya), 0x3f800000, np.uint32)))
    # quotients on atanf's range boundaries: y = c * x exactly (x a power of two)
    for xp in (0.5, 2.0, -4.0, 1024.0, -2.0 ** -20):
        c = bits(around(ATAN_CONST[2:], 2))
        for s in (1, -1):
            parts.append(records(f32(c * F32(xp) * F32(s)), np.full(len(c), xp, np.float32)))
    # random fill: any two bit patterns; moderate magnitudes (all of atanf's ranges); a strided sweep of y
    n = 60000
    parts.append(records(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                         rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)))
    parts.append(records(f32(rng.normal(0, 1, n) * np.exp(rng.uniform(-3, 3, n))), f32(rng.normal(0, 1, n))))
    ys = np.arange(0, 0x7f800001, 53003, dtype=np.uint32)
    xs = f32(np.where(np.arange(len(ys)) % 2 == 0, 3.0, -0.75))
    parts.append(records(ys ^ ((np.arange(len(ys), dtype=np.uint32) % 3 == 0).astype(np.uint32) << 31), xs))
    return np.concatenate(parts)


def grid_logf():
    edges = []
    for k in (-126, -100, -25, -2, -1, 0, 1, 2, 24, 100, 127):  # the 16 table intervals in several binades
        for j in range(17):
            u = LOGF_OFF + (j << 19) + (k << 23)
            if 0 < u < 0x7f800000:
                edges.append(u)
    u = np.concatenate([SPECIAL, around(edges, 1), around([0x3f800000, 0x00800000, 0x7f800000, LOGF_OFF], 3),
                        np.arange(1, 0x00800000, 104729, dtype=np.uint32),  # subnormals
                        np.arange(0, 0x7f800001, 21001, dtype=np.uint32),
                        np.arange(0x80000000, 0xff800001, 30000017, dtype=np.uint32)])
    return records(u.astype(np.uint32))


def grid_sincos():
    """|x| below 120: glibc_sincosf's stated domain (the render path evaluates angles in [0, 2 pi])."""
    lim = int(ubits(F32(120.0)).ravel()[0]) - 1
    k = np.arange(0, 77, dtype=np.float64)
    near = ubits(f32(np.concatenate([k * np.pi / 2, k * np.pi / 2 + np.pi / 4])))  # octant boundaries of the reduction
    near = near[(near <= lim - 4) & (near > 4)]
    u = np.concatenate([np.uint32([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, lim, lim | 0x80000000]),
                        both_signs(around([0x39800000, 0x3f490fdb, 0x3f400000, 0x40c90fdb], 3)),  # 2^-12, pi/4, 0.75, 2 pi
                        both_signs(around(near, 2)),
                        np.arange(0, lim, 10007, dtype=np.uint32),
                        np.arange(0, lim, 30011, dtype=np.uint32) | np.uint32(0x80000000)])
    return records(u.astype(np.uint32))


# ---------------------------------------------------------------- numeric
def grid_f2u():
    rng = np.random.default_rng(1203)
    named = f32([-0.0, 0.0, -0.5, 0.5, -1.0, 1.0, 255.0, 256.0, 257.0, 255.5, -255.0, -256.0, 65536.0, 2.0 ** 31,
                 2.0 ** 32, -2.0 ** 31, -2.0 ** 32, 9.2233715e18, -9.2233715e18, 2.0 ** 63, -2.0 ** 63, 2.0 ** 62,
                 2.0 ** 64, np.inf, -np.inf, np.nan, 1e-40, 2.0 ** 24, 2.0 ** 24 + 1, 3e9, -3e9, 4294967040.0])
    u = np.concatenate([SPECIAL, around(ubits(named), 2),
                        rng.integers(0, 2 ** 32, 40000, dtype=np.uint64).astype(np.uint32),
                        ubits(f32(rng.uniform(-2.0 ** 33, 2.0 ** 33, 30000))),
                        ubits(f32(rng.uniform(-300, 300, 20000))),
                        ubits(f32(np.exp2(rng.uniform(28, 66, 20000)) * rng.choice([-1.0, 1.0], 20000)))])
    return records(u.astype(np.uint32))


def grid_gmod():
    rng = np.random.default_rng(1204)
    two_pi = F32(6.2831855)
    a = np.concatenate([bits(SPECIAL), f32([-0.25, -1.0, -6.2831855, 6.2831855, 12.566371, -12.566371, 3.0, -3.0, 7.5, -7.5, 1e30,
                                            -1e30, 3.4e38, 1e-40, -1e-40, 1e-45, 0.99999994, -0.99999994, 2.0 ** 24, -2.0 ** 24,
                                            1.5, 2.5, -1.5, 1e-10, -1e-10])])
    b = f32([1.0, two_pi, 0.5, 3.0, -1.0, -3.0, 1e-40, 1e30, 0.1, 2.0 ** -126, np.inf, 0.0])
    aa, bb = cross(a, b)
    parts = [records(aa, bb)]
    m = rng.integers(-1000, 1000, 5000).astype(np.float32)
    for d in (F32(1), two_pi, F32(0.1), F32(3)):  # exact multiples and their neighbours
        p = f32(m * d)
        for q in (p, np.nextafter(p, F32(np.inf)), np.nextafter(p, F32(-np.inf))):
            parts.append(records(q, np.full(len(q), d, np.float32)))
    n = 60000
    parts.append(records(f32(rng.uniform(-50, 50, n)), f32(rng.choice([1.0, float(two_pi), 0.5, 3.0, 7.25], n))))
    parts.append(records(f32(rng.normal(0, 1, n) * np.exp(rng.uniform(-20, 20, n))), f32(np.exp(rng.uniform(-5, 5, n)))))
    return np.concatenate(parts)


def grid_gfract():
    rng = np.random.default_rng(1205)
    named = f32([-0.25, -1.0, 1.0, 3.0, -3.0, 7.5, -7.5, 1e30, -1e30, 1e-40, -1e-40, 1e-45, -1e-45, 0.99999994, -0.99999994,
                 2.0 ** 23, 2.0 ** 23 + 0.5, 2.0 ** 24, -2.0 ** 23 - 0.5, 1e-10, -1e-10, -5.9604645e-08, 8388607.5, -8388607.5])
    m = rng.integers(-100000, 100000, 10000).astype(np.float32)
    u = np.concatenate([SPECIAL, around(ubits(named), 1), around(ubits(m), 1),
                        ubits(f32(rng.uniform(-4, 4, 60000))),
                        ubits(f32(rng.normal(0, 1, 40000) * np.exp(rng.uniform(-30, 30, 40000)))),
                        rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)])
    return records(u.astype(np.uint32))


RNG_STATES = np.uint32([0, 1, 0xFFFFFFFF, 2463534242, 0x80000000, 0x7FFFFFFF, 2, 0x9E3779B9, 0x9E3779BB])
RNG_MAX = np.uint32([0, 1, 2, 255, 2 ** 31, 2 ** 32 - 1])


def grid_rng_float():
    rng = np.random.default_rng(1206)
    st = np.concatenate([RNG_STATES, np.arange(0, 4096, dtype=np.uint32) + np.uint32(2463534242),
                         rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)])
    return records(st)


def grid_rng_int():
    rng = np.random.default_rng(1207)
    s, m = cross(np.concatenate([RNG_STATES, rng.integers(0, 2 ** 32, 8000, dtype=np.uint64).astype(np.uint32)]), RNG_MAX)
    n = 50000
    return np.concatenate([records(s, m), records(rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                                                  rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))])


# ---------------------------------------------------------------- sampling
SAMPLE_EDGES = f32([0.0, 2.0 ** -24, 0.25, 0.5, ONE_M])
INNER = f32([0.0, 0.5, ONE_M])


def _sample_fill(seed, n):
    rng = np.random.default_rng(seed)
    return f32(rng.uniform(0, 1, n)).clip(0, ONE_M), f32(rng.uniform(0, 1, n)).clip(0, ONE_M)


def grid_sample2(seed=1208):
    x, y = cross(SAMPLE_EDGES, SAMPLE_EDGES)
    rx, ry = _sample_fill(seed, 50000)
    return records(np.concatenate([x, rx]), np.concatenate([y, ry]))


def grid_ring():
    x, y, i = cross(SAMPLE_EDGES, SAMPLE_EDGES, INNER)
    rng = np.random.default_rng(1209)
    rx, ry = _sample_fill(1210, 50000)
    ri = f32(rng.choice([0.0, 0.5, float(ONE_M), 0.25, 0.9], 50000))
    ri[::7] = f32(rng.uniform(0, 1, len(ri[::7]))).clip(0, ONE_M)
    return records(np.concatenate([x, rx]), np.concatenate([y, ry]), np.concatenate([i, ri]))


# ---------------------------------------------------------------- directions
def _dir(z, phi):
    z = np.float64(z)
    s = np.sqrt(max(0.0, 1.0 - z * z))
    return [s * np.cos(phi), s * np.sin(phi), z]


def direction_set():
    """Directions with z in {+-1, +-0, +-2^-12, +-1e-4, +-(1 - 2^-24)} and ordinary ones, axis-aligned ones included."""
    d = []
    for z in (1.0, 2.0 ** -12, 1e-4, float(ONE_M), 0.5, 0.8660254, 0.2):
        for sg in (1.0, -1.0):
            if z == 1.0:
                d.append([0.0, 0.0, sg])
            else:
                d.append(_dir(sg * z, 0.7))
                if z in (2.0 ** -12, 0.5):
                    d.append(_dir(sg * z, 2.5))
    d += [[0.6, 0.8, 0.0], [0.6, -0.8, -0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, -0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]]
    return f32(d)


def random_dirs(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return f32(v / np.linalg.norm(v, axis=1)[:, None])


ALPHAS = f32([0.0, 1e-4, np.nextafter(F32(1e-4), F32(1)), 1e-3, np.nextafter(F32(1e-3), F32(1)), 0.05, 0.5, 1.0, 1.5])
ETAS = f32([(1.0, 1.5), (1.5, 1.0), (1.5, 1.5), (1.33, 1.5), (2.0, 1.0)])  # (eta_outer, eta)
OTHER_ALPHA = F32(0.3)  # the alpha uap must not select


def np_dot(a, b):
    """dot3 as dmath.h / the oracle associate it, in float32."""
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def np_normalize(v):
    with np.errstate(all="ignore"):
        s = F32(1) / np.sqrt(np_dot(v, v))
    return v * s[:, None]


def shade_records(typ, uap, flags, rho, tau, eta, alpha, eta_outer, wo, c12, c13, c14):
    """Shading records (nart_hip.h): alpha is the selected roughness; the other one is OTHER_ALPHA."""
    n = len(wo)
    typ = np.broadcast_to(np.asarray(typ, np.uint32), (n,))
    uap = np.broadcast_to(np.asarray(uap, np.uint32), (n,))
    flags = np.broadcast_to(np.asarray(flags, np.uint32), (n,))
    alpha = np.broadcast_to(f32(alpha), (n,))
    r = np.zeros((n, W), np.float32)
    r[:, 0] = (typ | (uap << 8) | (flags << 16)).astype(np.uint32).view(np.float32)
    r[:, 1:4] = rho
    r[:, 4] = tau
    r[:, 5] = eta
    r[:, 6] = np.where(uap == 1, OTHER_ALPHA, alpha)
    r[:, 7] = np.where(uap == 1, alpha, OTHER_ALPHA)
    r[:, 8] = eta_outer
    r[:, 9:12] = wo
    r[:, 12] = c12
    r[:, 13] = c13
    r[:, 14] = c14
    return r


def rec_type(r):
    return ubits(r[:, 0]) & 0xFF


def rec_uap(r):
    return (ubits(r[:, 0]) >> 8) & 1


def rec_alpha(r):
    return np.where(rec_uap(r) == 1, r[:, 7], r[:, 6])


RHO = f32([0.8, 0.5, 0.25])
TAU = F32(0.9)


def _wi_for(wo, dirs):
    """For every wo: the direction set, reflect(wo), -wo and wo mirrored through the plane."""
    wos, wis = [], []
    for o in wo:
        w = np.concatenate([dirs, f32([[-o[0], -o[1], o[2]], [-o[0], -o[1], -o[2]], [o[0], o[1], -o[2]]])])
        wos.append(np.repeat(o[None, :], len(w), 0))
        wis.append(w)
    return np.concatenate(wos), np.concatenate(wis)


def critical_wo(azimuths=(0.0,)):
    """(eta_outer, eta) = (2, 1): sin_i = 2 sqrt(1 - wo.z^2) is 1 at wo.z ~ sqrt(3)/2.  Every float within 64
    ulps of it: sin_i moves by several ulps per ulp of wo.z, so it lands on exactly 1 and, on either side, on the
    nearest values it can take at all (1 - 2^-23 and 1 + 2^-22; the floats between are no 2 sqrt(1 - z * z))."""
    z = bits(around(ubits(F32(np.sqrt(0.75))), 64))
    s = np.sqrt(np.maximum(F32(0), F32(1) - z * z)).astype(np.float32)  # (s cos, s sin, z): unit up to rounding
    return np.concatenate([np.stack([f32(s * F32(np.cos(a))), f32(s * F32(np.sin(a))), z], 1) for a in azimuths])


def grid_eval_pairs():
    """Inputs of bxdf_f, bxdf_pdf and bxdf_f_pdf: (wo, wi) pairs."""
    rng = np.random.default_rng(1211)
    dirs = direction_set()
    parts = []
    regular = dirs[dirs[:, 2] != 0]
    flat = dirs[dirs[:, 2] == 0]

    def add(typ, wo, wi, alpha, uap, eta_pair):
        parts.append(shade_records(typ, uap, 0, RHO, TAU, eta_pair[:, 1], alpha, eta_pair[:, 0], wo, wi[:, 0], wi[:, 1], wi[:, 2]))

    def crossed(typ, wo_set, alphas, etas):
        wo, wi = _wi_for(wo_set, dirs)
        i, a, u, e = cross(np.arange(len(wo)), alphas, np.uint32([0, 1]), np.arange(len(etas)))
        add(typ, wo[i], wi[i], a, u, etas[e])

    for typ in (B_DIEL, B_TS):
        crossed(typ, regular, ALPHAS[1:], ETAS)
        # wo.z == +-0 and alpha == 0 divide zero by zero (a NaN pdf or D): present, but not the bulk
        crossed(typ, flat, f32([0.05, 0.5]), ETAS[:3])
        crossed(typ, regular[::4], ALPHAS[:1], ETAS[:3])
        # the critical angle of (2, 1), from either side of the surface
        cw = critical_wo()
        for sg in (F32(1), F32(-1)):
            wo, wi = _wi_for(cw * f32([1, 1, sg]), dirs[::3])
            add(typ, wo, wi, F32(0.05), 0, np.repeat(ETAS[4:5], len(wo), 0))
        # seeded directions
        n = 4096
        wo, wi = random_dirs(rng, n), random_dirs(rng, n)
        add(typ, wo, wi, f32(rng.choice(ALPHAS[1:], n)), rng.integers(0, 2, n).astype(np.uint32), ETAS[rng.integers(0, 5, n)])
        # ... and physically consistent pairs: wi the mirror direction / the refraction about a random half vector
        wh = random_dirs(rng, n)
        wh[:, 2] = np.abs(wh[:, 2])
        d = np_dot(wo, wh)
        add(typ, wo, f32(wh * (F32(2) * d)[:, None] - wo), f32(rng.choice(ALPHAS[5:], n)), 0, ETAS[rng.integers(0, 5, n)])
    for typ in (B_LAMBERT, B_SPECULAR, B_SPECDIEL):
        crossed(typ, dirs, ALPHAS[6:7], ETAS[:3])
        n = 4096
        add(typ, random_dirs(rng, n), random_dirs(rng, n), F32(0.5), 0, ETAS[rng.integers(0, 5, n)])
    return np.concatenate(parts)


def _oracle_eval(op, x):
    import oracle
    return oracle.eval(op, x)


def fresnel_of_wh(r):
    """Fr of each bxdf_sample_f record as B_DIEL computes it: the oracle's sample_wh for the case, then the
    oracle's fresnel on |dot(wh, wo)| with the etas swapped below the surface.  B_SPECDIEL: on |wo.z|."""
    typ = rec_type(r)
    wo = r[:, 9:12]
    q = np.zeros((len(r), W), np.float32)
    q[:, 0], q[:, 1], q[:, 2] = r[:, 13], r[:, 14], rec_alpha(r)
    q[:, 3] = np.uint32(1).view(np.float32)
    q[:, 4:7] = wo
    with np.errstate(all="ignore"):
        wh = _oracle_eval("sample_wh", q)[:, :3]
        c = np.abs(np_dot(wh, wo))
    c = np.where(typ == B_SPECDIEL, np.abs(wo[:, 2]), c)
    below = wo[:, 2] < 0
    eo = np.where(below, r[:, 5], r[:, 8])
    ei = np.where(below, r[:, 8], r[:, 5])
    return _oracle_eval("fresnel", records(eo, ei, c))[:, 0]


def grid_sample_f():
    """Inputs of bxdf_sample_f.  s1 (B_DIEL) and sample.x (B_SPECDIEL) are compared with the case's own Fresnel
    term: the fixed values 0, 0.5, 1 - 2^-24, then that term and the floats on either side of it."""
    rng = np.random.default_rng(1212)
    dirs = direction_set()
    regular = dirs[dirs[:, 2] != 0]
    flat = dirs[dirs[:, 2] == 0]
    FIXED = f32([0.0, 0.5, ONE_M])
    parts = []

    def add(typ, wo, alpha, uap, eta_pair, s1, sx, sy, flags):
        parts.append(shade_records(typ, uap, flags, RHO, TAU, eta_pair[:, 1], alpha, eta_pair[:, 0], wo, s1, sx, sy))

    def with_fr(typ, wo, alpha, uap, eta_pair, sx, sy, flags):
        """The case at each fixed value of its compared field, then at its own Fr and Fr's neighbours."""
        col = 12 if typ == B_DIEL else 13
        base = shade_records(typ, uap, flags, RHO, TAU, eta_pair[:, 1], alpha, eta_pair[:, 0], wo, F32(0.5), sx, sy)
        for v in FIXED:
            b = base.copy()
            b[:, col] = v
            parts.append(b)
        fr = fresnel_of_wh(base)  # (B_DIEL: sample decides wh, hence Fr, and s1 follows; B_SPECDIEL: Fr of |wo.z|)
        for v in (np.nextafter(fr, F32(-np.inf)), fr, np.nextafter(fr, F32(np.inf))):
            b = base.copy()
            b[:, col] = v
            parts.append(b[np.isfinite(v)])

    # B_DIEL: directions x roughness x uap x etas x sample
    wo_i, a, u, e, sx, sy = cross(np.arange(len(regular)), ALPHAS[1:], np.uint32([0, 1]), np.arange(5),
                                  f32([0.0, 0.5, ONE_M]), f32([0.25, 0.7]))
    fl = np.where(np.arange(len(wo_i)) % 2 == 0, 0, 0xFF).astype(np.uint32)
    fl = np.where(e == 2, np.where((np.arange(len(wo_i)) // 2) % 2 == 0, 0, 0xFF), fl).astype(np.uint32)
    with_fr(B_DIEL, regular[wo_i], a, u, ETAS[e], sx, sy, fl)
    # equal etas: both incoming flags for every direction (the branch ORs into them)
    for f in (0, 0xFF):
        add(B_DIEL, dirs, F32(0.05), 0, np.repeat(ETAS[2:3], len(dirs), 0), F32(0.5), F32(0.5), F32(0.25), f)
        add(B_SPECDIEL, dirs, F32(0.0), 0, np.repeat(ETAS[2:3], len(dirs), 0), F32(0.5), F32(0.5), F32(0.25), f)
    # wo.z == +-0 and alpha == 0 (NaN-prone): a few
    wo_i, a, e = cross(np.arange(len(flat)), f32([0.05, 0.5]), np.arange(5))
    add(B_DIEL, flat[wo_i], a, 0, ETAS[e], F32(0.5), F32(0.5), F32(0.25), 0)
    add(B_TS, flat[wo_i], a, 0, ETAS[e], F32(0.5), F32(0.5), F32(0.25), 0)
    wo_i, u, e = cross(np.arange(len(regular)), np.uint32([0, 1]), np.arange(5))
    add(B_DIEL, regular[wo_i], F32(0), u, ETAS[e], F32(0.5), F32(0.5), F32(0.25), 0xFF)
    add(B_TS, regular[wo_i], F32(0), u, ETAS[e], F32(0.5), F32(0.5), F32(0.25), 0xFF)
    # wo = (0, 0, +-1): sample_wh's T1 (the dielectric picks (1, 0, 0); Torrance-Sparrow normalizes a zero vector)
    up = f32([[0, 0, 1], [0, 0, -1]])
    wo_i, a, e, sx = cross(np.arange(2), ALPHAS[1:], np.arange(5), f32([0.0, 0.5, ONE_M]))
    add(B_DIEL, up[wo_i], a, 0, ETAS[e], F32(0.5), sx, F32(0.25), 0)
    add(B_TS, up[wo_i[::8]], a[::8], 0, ETAS[e[::8]], F32(0.5), sx[::8], F32(0.25), 0)
    # the critical angle of (2, 1), smooth and nearly smooth
    cw = critical_wo((0.0, 0.7, 1.3, 2.5, 4.0, 5.5))
    for sg in (F32(1), F32(-1)):
        w = cw * f32([1, 1, sg])
        for et in (ETAS[4:5], ETAS[1:2]):
            with_fr(B_SPECDIEL, w, F32(0), 0, np.repeat(et, len(w), 0), F32(0.5), F32(0.25), 0)
            for al in (F32(1e-4), F32(1e-3), F32(0.05)):
                with_fr(B_DIEL, w, al, 0, np.repeat(et, len(w), 0), F32(0.5), F32(0.25), 0)
    # B_TS: directions x roughness x uap x etas x sample
    wo_i, a, u, e, sx, sy = cross(np.arange(len(regular)), ALPHAS[1:], np.uint32([0, 1]), np.arange(5),
                                  f32([0.0, 0.5, ONE_M]), f32([0.0, 0.25, 0.7]))
    add(B_TS, regular[wo_i], a, u, ETAS[e], F32(0.5), sx, sy, np.where(np.arange(len(wo_i)) % 2 == 0, 0, 0xFF))
    # B_SPECDIEL, B_SPECULAR, B_LAMBERT
    wo_i, e = cross(np.arange(len(dirs)), np.arange(5))
    with_fr(B_SPECDIEL, dirs[wo_i], F32(0), 0, ETAS[e], F32(0.5), F32(0.25), np.where(np.arange(len(wo_i)) % 2 == 0, 0, 0xFF))
    for f in (0, 0xFF):
        add(B_SPECULAR, dirs[wo_i], F32(0), 0, ETAS[e], F32(0.5), F32(0.5), F32(0.25), f)
    sx, sy = cross(SAMPLE_EDGES, SAMPLE_EDGES)
    add(B_LAMBERT, np.repeat(dirs[:1], len(sx), 0), F32(0), 0, np.repeat(ETAS[:1], len(sx), 0), F32(0.5), sx, sy, 0xFF)
    # seeded directions, 4096 per type
    n = 4096
    for typ in (B_LAMBERT, B_SPECULAR, B_SPECDIEL, B_DIEL, B_TS):
        s1, sx = _sample_fill(1213 + typ, n)
        sy = _sample_fill(1220 + typ, n)[0]
        al = f32(rng.choice(ALPHAS[1:], n))
        al[::2] = f32(np.exp(rng.uniform(np.log(2e-4), np.log(2.0), len(al[::2]))))
        add(typ, random_dirs(rng, n), al, rng.integers(0, 2, n).astype(np.uint32), ETAS[rng.integers(0, 5, n)], s1, sx, sy,
            rng.choice(np.uint32([0, 0xFF]), n))
    return np.concatenate(parts)


def grid_sample_wh():
    rng = np.random.default_rng(1214)
    dirs = np.concatenate([direction_set(), f32([[0, 0, 1], [0, 0, -1]])])
    sx, sy, a, d, w = cross(SAMPLE_EDGES, SAMPLE_EDGES, ALPHAS[1:], np.uint32([0, 1]), np.arange(len(dirs)))
    r = records(sx, sy, a, d)
    r[:, 4:7] = dirs[w]
    n = 50000
    rx, ry = _sample_fill(1215, n)
    q = records(rx, ry, f32(np.exp(rng.uniform(np.log(1e-4), np.log(2.0), n))), rng.integers(0, 2, n).astype(np.uint32))
    q[:, 4:7] = random_dirs(rng, n)
    return np.concatenate([r, q])


def grid_fresnel():
    rng = np.random.default_rng(1216)
    # cosines: zeros, ones, grazing, and beyond 1 (clamped by the function)
    cs = f32([0.0, -0.0, 1.0, -1.0, 2.0 ** -12, -2.0 ** -12, 1e-4, -1e-4, ONE_M, -ONE_M, 1.5, -1.5, 1e-6, 0.5,
              np.nextafter(F32(1), F32(2)), -np.nextafter(F32(1), F32(2)), 2.0, -2.0, 1e30, -1e30, np.inf, -np.inf])
    dense = f32([(4.0, 1.0), (3.0, 2.0), (2.5, 1.0), (1.25, 1.0), (3.0, 1.0), (1.75, 1.0), (1.5, 1.33), (2.0, 1.5)])
    e = np.concatenate([ETAS, ETAS[:, ::-1], dense, dense[:, ::-1],
                        f32([(1.0, 1.0), (2.0, 2.0), (1.33, 1.33), (1.0, 1.0000001), (1.5, 1.4999999)])])
    i, c = cross(np.arange(len(e)), cs)
    parts = [records(e[i, 0], e[i, 1], c)]
    # the critical angle of every pair that has one (eta_o > eta_i): sin_i = (eta_o / eta_i) sqrt(1 - c^2)
    # crosses 1 at c = sqrt(1 - (eta_i / eta_o)^2); every float within 64 ulps of it, both signs
    for eo, ei in e[e[:, 0] > e[:, 1]]:
        c = bits(both_signs(around(ubits(F32(np.sqrt(1.0 - (float(ei) / float(eo)) ** 2))), 64)))
        parts.append(records(np.full(len(c), eo, np.float32), np.full(len(c), ei, np.float32), c))
    n = 60000
    ee = e[rng.integers(0, len(e), n)]
    re = np.where(rng.uniform(size=n)[:, None] < 0.5, ee, f32(rng.uniform(1, 2.5, (n, 2))))
    parts.append(records(re[:, 0], re[:, 1], f32(rng.uniform(-1, 1, n))))
    return np.concatenate(parts)


GRIDS = {
    "acosf": grid_acosf, "atanf": grid_atanf, "atan2f": grid_atan2f, "logf": grid_logf, "logf_lds": grid_logf,
    "sincos": grid_sincos, "f2u32": grid_f2u, "f2u8": grid_f2u, "gmod": grid_gmod, "gfract": grid_gfract,
    "rng_float": grid_rng_float, "rng_int": grid_rng_int, "uniform_sample_disk": grid_sample2,
    "uniform_sample_ring": grid_ring, "cosine_sample_hemisphere": grid_sample2, "uniform_sample_sphere": grid_sample2,
    "sample_wh": grid_sample_wh, "fresnel": grid_fresnel, "bxdf_f": grid_eval_pairs, "bxdf_pdf": grid_eval_pairs,
    "bxdf_f_pdf": grid_eval_pairs, "bxdf_sample_f": grid_sample_f,
}
LIBM_OPS = ("acosf", "atanf", "atan2f", "logf", "logf_lds", "sincos")
SHADING_OPS = ("fresnel", "bxdf_f", "bxdf_pdf", "bxdf_f_pdf", "bxdf_sample_f")
# output words each op defines (the others are 0 on both sides)
OUT_WORDS = {"sincos": 2, "rng_float": 2, "rng_int": 2, "uniform_sample_disk": 2, "uniform_sample_ring": 3,
             "cosine_sample_hemisphere": 4, "uniform_sample_sphere": 3, "sample_wh": 3, "bxdf_f": 3, "bxdf_f_pdf": 4,
             "bxdf_sample_f": 9}


@functools.lru_cache(maxsize=None)
def _grid(fn):
    g = np.ascontiguousarray(fn(), np.float32)
    g.setflags(write=False)
    return g


def grid(op):
    """The op's input records (read-only, computed once per process)."""
    return _grid(GRIDS[op])


@functools.lru_cache(maxsize=None)
def expected(op):
    """The oracle's outputs on grid(op) (read-only, computed once per process)."""
    e = _oracle_eval(op, grid(op))
    e.setflags(write=False)
    return e


# output words that hold integers as bits: always compared bit for bit (never read as NaN)
INT_WORDS = {"f2u32": (0,), "f2u8": (0,), "rng_float": (1,), "rng_int": (0, 1), "bxdf_sample_f": (7,)}


def nan_words(op, out):
    """Which output words hold a float NaN (integer words never do)."""
    m = np.isnan(out)
    for k in INT_WORDS.get(op, ()):
        m[:, k] = False
    return m


def compare(op, got, want):
    """Indices of records where got departs from want: bit equality where want is not NaN, NaN where it is
    (x86 and the GPU differ in the sign and payload of a generated NaN; the reference fixes neither)."""
    wn = nan_words(op, want)
    bad = np.where(wn, ~nan_words(op, got), ubits(got).reshape(got.shape) != ubits(want).reshape(want.shape))
    return np.nonzero(bad.any(axis=1))[0]


def describe(op, x, got, want, idx, limit=5):
    """The first few failing cases: inputs and both outputs in hex."""
    k = OUT_WORDS.get(op, 1)
    lines = ["%s: %d of %d cases differ" % (op, len(idx), len(x))]
    for i in idx[:limit]:
        lines.append("  case %d in  %s" % (i, " ".join("%08x" % v for v in ubits(x[i])[:15])))
        lines.append("         got  %s" % " ".join("%08x" % v for v in ubits(got[i])[:k]))
        lines.append("         want %s" % " ".join("%08x" % v for v in ubits(want[i])[:k]))
    return "\n".join(lines)
