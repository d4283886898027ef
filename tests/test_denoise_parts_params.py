"""denoise_parts_error (csrc/host/stage_params.h), checked on the CPU against a restatement of its rules:
which message, and which rule comes first -- the count, the images, the denoiser's parameters, the guide
parameters -- over cases that break one rule alone and cases that break it together with later ones."""
import itertools
import math

import numpy as np
import pytest

import denoise_parts_native

F = np.float32
DENOISE = ["iterations", "normal_squarings", "sigma_color", "sigma_depth", "depth_eps", "sigma_coverage", "albedo_floor"]
DEFAULTS = dict(iterations=5, normal_squarings=5, sigma_color=4.0, sigma_depth=1.0, depth_eps=1e-3, sigma_coverage=0.05,
                albedo_floor=0.01)
GUIDE_DEFAULT = 8


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return denoise_parts_native.build_checker(tmp_path_factory.mktemp("denoise_parts_params"))


def _tok(name, v):
    if name in ("iterations", "normal_squarings"):
        return "%d" % v
    v = float(F(v))
    return "nan" if math.isnan(v) else ("inf" if v > 0 else "-inf") if math.isinf(v) else v.hex()


def _line(n_parts, given, dp, gp):
    return "error %d %d %s %s" % (n_parts, 1 if given else 0,
                                  "null" if dp is None else " ".join(_tok(f, dp[f]) for f in DENOISE),
                                  "null" if gp is None else "%d" % gp)


def expected(n_parts, given, dp, gp):
    """The restatement: the first broken rule's message, or ""."""
    d = DEFAULTS if dp is None else dp
    if n_parts < 1 or n_parts > 9:
        return "n_parts must be 1..9"
    if not given:
        return "the part images, the guide images and the denoised images are required"
    if d["iterations"] < 1 or d["iterations"] > 8:
        return "denoise iterations must be 1..8"
    if d["normal_squarings"] > 16:
        return "denoise normal_squarings must be <= 16"
    if not all(F(d[f]) > 0 for f in DENOISE[2:]):
        return "denoise sigmas, depth_eps and albedo_floor must be > 0"
    if gp is not None and gp > 10:
        return "max_follow must be 0..10"
    return ""


def test_rules_and_their_order(checker):
    counts = [0, 1, 5, 9, 10, 0xFFFFFFFF]
    dps = [None, dict(DEFAULTS), dict(DEFAULTS, iterations=0), dict(DEFAULTS, iterations=9),
           dict(DEFAULTS, normal_squarings=17), dict(DEFAULTS, sigma_color=0.0), dict(DEFAULTS, albedo_floor=float("nan")),
           dict(DEFAULTS, iterations=9, sigma_depth=-1.0), dict(DEFAULTS, iterations=8, normal_squarings=16)]
    gps = [None, 0, 8, 10, 11]
    cases = list(itertools.product(counts, [True, False], dps, gps))
    answers = checker([_line(*c) for c in cases])
    messages = set()
    for c, (message, fields, follow) in zip(cases, answers):
        assert message == expected(*c), (c, message)
        messages.add(message)
        # dp and gp are copied out (null: the defaults) whatever rule breaks
        want = DEFAULTS if c[2] is None else c[2]
        for f, g in zip(DENOISE, fields.split()):
            if f in ("iterations", "normal_squarings"):
                assert int(g) == want[f]
            else:
                a, b = F(float.fromhex(g)), F(want[f])
                assert (np.isnan(a) and np.isnan(b)) or a == b
        assert int(follow) == (GUIDE_DEFAULT if c[3] is None else c[3])
    assert len(messages) == 7  # every rule, and no error, was reached
