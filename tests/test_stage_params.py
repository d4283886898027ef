"""The parameter structs of the whole-image stages (csrc/host/stage_params.h), checked on the CPU.

The defaults are compared with the values include/nart_hip.h documents; every X_params_error and the
three checks of the render parameters with a restatement of the rules -- which message, and which rule
first -- over cases that break one rule alone and cases that break it together with a later one; the
adaptive levels and the cascade levels with their definitions."""
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "nart_hip.h")
F = np.float32
INF, NAN = float("inf"), float("nan")

# field order of each struct (include/nart_hip.h); "spp" is the adaptive check's second argument
FIELDS = {
    "denoise": ["iterations", "normal_squarings", "sigma_color", "sigma_depth", "depth_eps", "sigma_coverage", "albedo_floor"],
    "guide": ["max_follow"],
    "adaptive": ["min_spp", "growth", "threshold", "floor"],
    "cascade": ["layers", "start", "base", "kappa"],
    "matte": ["kind", "ranks"],
}
INTS = {"iterations", "normal_squarings", "max_follow", "min_spp", "growth", "layers", "kind", "ranks", "spp",
        "image_width", "image_height"}


def _tok(name, v):
    if name in INTS:
        return "%d" % v
    v = float(F(v))
    return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf") if math.isinf(v) else v.hex()


def _same(name, got, want):
    if name in INTS:
        return int(got) == int(want)
    a, b = F(float.fromhex(got)), F(want)
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("stage_params") / "stage_params_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "native", "stage_params_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split("|") for a in answers]
    return ask


def _ask_struct(checker, what, cases):
    """cases: dicts of the struct's fields (None: a null pointer), the adaptive ones with "spp".  Returns
    (message, levels) per case, having checked that `out` holds the input's fields."""
    lines = []
    for v in cases:
        head = what + (" %d" % v["spp"] if what == "adaptive" else "")
        lines.append(head + " " + ("null" if v.get("null") else " ".join(_tok(f, v[f]) for f in FIELDS[what])))
    got = []
    for v, (message, fields, levels) in zip(cases, checker(lines)):
        want = DEFAULTS[what] if v.get("null") else v
        for f, g in zip(FIELDS[what], fields.split()):
            assert _same(f, g, want[f]), (what, v, f, g)
        got.append((message, levels.split()))
    return got


# ------------------------------------------------------------------ the defaults, as the header documents them
DEFAULTS = {
    "denoise": dict(iterations=5, normal_squarings=5, sigma_color=4.0, sigma_depth=1.0, depth_eps=1e-3,
                    sigma_coverage=0.05, albedo_floor=0.01),
    "guide": dict(max_follow=8),
    "adaptive": dict(min_spp=16, growth=4, threshold=0.1, floor=0.01),
    "cascade": dict(layers=6, start=1.0, base=8.0, kappa=2.0),
    "matte": dict(kind=0, ranks=6),
}


def _documented(struct):
    """{field: default} of `typedef struct nart_<struct>_params` from the comments of include/nart_hip.h."""
    text = open(HEADER).read()
    body = re.search(r"typedef struct nart_%s_params \{(.*?)\} nart_%s_params;" % (struct, struct), text, re.S).group(1)
    names = re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", body, re.M)
    values = re.findall(r"default\s+(\S+)\s*\*/", body)
    assert len(names) == len(values) == len(FIELDS[struct]), (struct, names, values)
    return {n: 0.0 if v == "mesh" else float(v) for n, v in zip(names, values)}  # NART_MATTE_MESH is 0


def test_defaults_are_the_documented_ones(checker):
    (answer,) = checker(["defaults"])
    assert len(answer) == 5
    for struct, fields in zip(("denoise", "guide", "adaptive", "cascade", "matte"), answer):
        doc = _documented(struct)
        assert list(doc) == FIELDS[struct]
        for f, g in zip(FIELDS[struct], fields.split()):
            assert _same(f, g, doc[f]), (struct, f, g, doc[f])
            assert _same(f, g, DEFAULTS[struct][f]), (struct, f)
    # a null pointer is the defaults, and they are valid
    for struct in FIELDS:
        (got,) = _ask_struct(checker, struct, [dict(null=True, spp=64)])
        assert got[0] == "", (struct, got)


# ------------------------------------------------------------------ the rules, restated
def _pos(v):  # "> 0" as the C comparison has it: false for a NaN
    return F(v) > 0


def _finite(v):
    return bool(np.isfinite(F(v)))


def restate_denoise(v):
    if not 1 <= v["iterations"] <= 8:
        return "denoise iterations must be 1..8"
    if v["normal_squarings"] > 16:
        return "denoise normal_squarings must be <= 16"
    if not all(_pos(v[f]) for f in ("sigma_color", "sigma_depth", "depth_eps", "sigma_coverage", "albedo_floor")):
        return "denoise sigmas, depth_eps and albedo_floor must be > 0"
    return ""


def restate_guide(v):
    return "max_follow must be 0..10" if v["max_follow"] > 10 else ""


def restate_adaptive(v):
    if v["min_spp"] < 2:
        return "adaptive min_spp must be >= 2 (one sample has no variance)"
    if v["spp"] < 2:
        return "adaptive sampling needs spp >= 2 (one sample has no variance)"
    if not 2 <= v["growth"] <= 16:
        return "adaptive growth must be in 2..16"
    if not F(v["threshold"]) >= 0:
        return "adaptive threshold must be >= 0 (+inf: nothing refines)"
    if not (_pos(v["floor"]) and _finite(v["floor"])):
        return "adaptive floor must be finite and > 0"
    return ""


def cascade_levels(v):
    """b_j = start * base^j by repeated float multiplication: (message, levels)."""
    levels, b = [], F(v["start"])
    with np.errstate(over="ignore"):
        for j in range(v["layers"]):
            if not np.isfinite(b):
                return "a cascade level is not finite", []
            if j and not b > levels[-1]:
                return "the cascade levels do not increase (start too small for base)", []
            levels.append(b)
            b = F(b * F(v["base"]))
    return "", levels


def restate_cascade(v):
    if not 2 <= v["layers"] <= 8:
        return "cascade layers must be in 2..8"
    if not (_finite(v["start"]) and _pos(v["start"])):
        return "cascade start must be finite and > 0"
    if not (_finite(v["base"]) and F(v["base"]) > 1):
        return "cascade base must be finite and > 1"
    if not (_finite(v["kappa"]) and _pos(v["kappa"])):
        return "cascade kappa must be finite and > 0"
    return cascade_levels(v)[0]


def restate_matte(v):
    if v["kind"] not in (0, 1):
        return "unknown matte id kind"
    if not 2 <= v["ranks"] <= 8 or v["ranks"] % 2:
        return "matte ranks must be even and in 2..8"
    return ""


RESTATE = dict(denoise=restate_denoise, guide=restate_guide, adaptive=restate_adaptive, cascade=restate_cascade,
               matte=restate_matte)

# Per struct, rule by rule in the order the rules are checked: the message and ways to break that rule alone.
BREAKS = {
    "denoise": [
        ("denoise iterations must be 1..8", [dict(iterations=0), dict(iterations=9)]),
        ("denoise normal_squarings must be <= 16", [dict(normal_squarings=17)]),
        ("denoise sigmas, depth_eps and albedo_floor must be > 0",
         [{f: bad} for f in FIELDS["denoise"][2:] for bad in (0.0, -1.0, NAN)]),
    ],
    "guide": [("max_follow must be 0..10", [dict(max_follow=11), dict(max_follow=0xFFFFFFFF)])],
    "adaptive": [
        ("adaptive min_spp must be >= 2 (one sample has no variance)", [dict(min_spp=1), dict(min_spp=0)]),
        ("adaptive sampling needs spp >= 2 (one sample has no variance)", [dict(spp=1), dict(spp=0)]),
        ("adaptive growth must be in 2..16", [dict(growth=1), dict(growth=17)]),
        ("adaptive threshold must be >= 0 (+inf: nothing refines)", [dict(threshold=-1e-3), dict(threshold=NAN)]),
        ("adaptive floor must be finite and > 0", [dict(floor=0.0), dict(floor=-1.0), dict(floor=INF), dict(floor=NAN)]),
    ],
    "cascade": [
        ("cascade layers must be in 2..8", [dict(layers=1), dict(layers=9)]),
        ("cascade start must be finite and > 0", [dict(start=0.0), dict(start=-1.0), dict(start=INF), dict(start=NAN)]),
        ("cascade base must be finite and > 1", [dict(base=1.0), dict(base=0.5), dict(base=INF), dict(base=NAN)]),
        ("cascade kappa must be finite and > 0", [dict(kappa=0.0), dict(kappa=-2.0), dict(kappa=INF), dict(kappa=NAN)]),
    ],
    "matte": [
        ("unknown matte id kind", [dict(kind=2)]),
        ("matte ranks must be even and in 2..8", [dict(ranks=0), dict(ranks=1), dict(ranks=3), dict(ranks=7), dict(ranks=10)]),
    ],
}
# valid values at the edges of the rules
VALID = {
    "denoise": [dict(iterations=1), dict(iterations=8), dict(normal_squarings=16), dict(normal_squarings=0),
                dict(sigma_color=INF), dict(depth_eps=1e-30)],
    "guide": [dict(max_follow=0), dict(max_follow=10)],
    "adaptive": [dict(min_spp=2), dict(spp=2), dict(growth=2), dict(growth=16), dict(threshold=0.0), dict(threshold=INF),
                 dict(floor=1e-30)],
    "cascade": [dict(layers=2), dict(layers=8), dict(start=1e-30), dict(base=1.0 + 2.0 ** -23), dict(kappa=1e-30)],
    "matte": [dict(kind=1), dict(ranks=2), dict(ranks=8), dict(ranks=4)],
}


def _base(struct):
    v = dict(DEFAULTS[struct])
    if struct == "adaptive":
        v["spp"] = 64
    return v


@pytest.mark.parametrize("struct", sorted(FIELDS))
def test_first_broken_rule_decides_the_message(checker, struct):
    rules = BREAKS[struct]
    cases, want = [], []
    for i, (message, ways) in enumerate(rules):
        for way in ways:  # this rule alone
            cases.append(dict(_base(struct), **way))
            want.append(message)
        for later_message, later_ways in rules[i + 1:]:  # and together with every later rule
            for way, later in itertools.product(ways, later_ways):
                cases.append(dict(_base(struct), **later, **way))
                want.append(message)
    for way in VALID[struct]:
        cases.append(dict(_base(struct), **way))
        want.append("")
    assert len(cases) > len(rules)
    for v, w, (message, _levels) in zip(cases, want, _ask_struct(checker, struct, cases)):
        assert RESTATE[struct](v) == w, (struct, v)  # the restatement agrees with the table
        assert message == w, (struct, v, message)


# ------------------------------------------------------------------ the levels
def adaptive_levels(min_spp, growth, spp):
    levels, L = [], min_spp
    while L < spp and len(levels) + 1 < 32:
        levels.append(L)
        L = min(L * growth, spp)
    return levels + [spp]


def test_adaptive_levels(checker):
    top = 0xFFFFFFFF
    cases = [(16, 4, 64), (16, 4, 16), (64, 4, 16), (2, 2, 2),  # min_spp >= spp: the one level spp
             (2, 2, 1024), (2, 2, 1000), (3, 16, 100000), (16, 16, 4096), (16, 16, 4097),
             (2, 2, top), (2, 2, 1 << 31), (3, 2, top),  # 32 levels at the most
             (1 << 28, 16, top), (1 << 31, 2, top), (top - 1, 16, top), (0x10000001, 16, top)]  # L * growth beyond 32 bits
    got = _ask_struct(checker, "adaptive", [dict(min_spp=m, growth=g, threshold=0.1, floor=0.01, spp=s) for m, g, s in cases])
    for (m, g, s), (message, levels) in zip(cases, got):
        levels = [int(x) for x in levels]
        assert message == "" and levels == adaptive_levels(m, g, s), (m, g, s, levels)
        assert levels[-1] == s and len(levels) <= 32 and all(a < b for a, b in zip(levels, levels[1:]))
        assert all(b == min(a * g, s) for a, b in zip(levels, levels[1:-1]))
        assert levels[0] == (m if m < s else s)
    by_case = {c: [int(x) for x in l] for c, (_m, l) in zip(cases, got)}
    assert by_case[(64, 4, 16)] == [16] and by_case[(16, 4, 64)] == [16, 64]
    assert len(by_case[(2, 2, top)]) == 32 and by_case[(2, 2, top)][30:] == [1 << 31, top]
    assert len(by_case[(3, 2, top)]) == 32 and by_case[(3, 2, top)][30:] == [3 << 30, top]  # the cap cuts the doubling short
    assert by_case[(1 << 28, 16, top)] == [1 << 28, top] and by_case[(0x10000001, 16, top)] == [0x10000001, top]


def test_cascade_levels(checker):
    tiny = 2.0 ** -149  # the least denormal: times 1.25 it rounds to itself
    cases = [dict(layers=6, start=1.0, base=8.0), dict(layers=8, start=0.01, base=3.7), dict(layers=2, start=1e30, base=1e5),
             dict(layers=3, start=1e30, base=1e5),  # 1e40 is not a float
             dict(layers=8, start=1e10, base=1e5), dict(layers=2, start=tiny, base=1.25),
             dict(layers=8, start=tiny, base=1.25), dict(layers=3, start=1.0, base=1.0 + 2.0 ** -23),
             dict(layers=8, start=3e38, base=1.0 + 2.0 ** -23)]
    cases = [dict(c, kappa=2.0) for c in cases]
    messages = []
    for v, (message, levels) in zip(cases, _ask_struct(checker, "cascade", cases)):
        want_message, want = cascade_levels(v)
        assert message == want_message, (v, message)
        assert [F(float.fromhex(x)) for x in levels] == want, (v, levels)
        assert len(levels) == (0 if message else v["layers"])
        messages.append(message)
    assert messages[3] == messages[4] == "a cascade level is not finite"
    assert messages[5] == messages[6] == "the cascade levels do not increase (start too small for base)"
    assert messages[:3] == ["", "", ""] and messages[7] == ""


# ------------------------------------------------------------------ what the stages need of the render parameters
def test_render_parameter_checks(checker):
    size = "imageWidth, imageHeight and filterWidth must be > 0"
    bad_sizes = [(0, 24, 2.0), (32, 0, 2.0), (32, 24, 0.0), (32, 24, -1.0), (32, 24, NAN), (0, 0, 0.0)]
    lines, want = [], []
    for w, h, fw in bad_sizes + [(32, 24, 2.0), (1, 1, 1e-30)]:
        ok = w > 0 and h > 0 and F(fw) > 0
        lines.append("image %d %d %s" % (w, h, _tok("filter_width", fw)))
        want.append("" if ok else size)
        for spp in (0, 1):  # the size rule comes before the cascade's own
            lines.append("cascade_frame %d %d %s %d" % (w, h, _tok("filter_width", fw), spp))
            want.append(size if not ok else "the cascade needs spp >= 1" if spp < 1 else "")
    for spp in (0, 1, 2, 3):
        lines.append("variance %d" % spp)
        want.append("sample variance needs spp >= 2" if spp < 2 else "")
    got = [a[0] for a in checker(lines)]
    assert got == want, [(l, g, w) for l, g, w in zip(lines, got, want) if g != w]
    assert set(want) == {"", size, "the cascade needs spp >= 1", "sample variance needs spp >= 2"}
