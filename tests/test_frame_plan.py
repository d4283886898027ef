"""What a frame produces (csrc/host/frame_plan.h plan_frame), checked on the CPU.

plan_frame is compared with a restatement of the rules -- which requests are refused, with which
code and message and which rule first; else the list of tile outputs in delivery order, the passes a
batch runs after the beauty's splat, whether the path kernel runs and the extra record memory -- over
every combination of what can be asked for."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -6
PATH, VOLUME = 0, 1
BEAUTY, ALBEDO, NORMAL, MOMENT, LAYER, PLANE = range(6)
CASCADE_PASS, MOMENT_PASS, FIRST_HIT_PASS, MATTE_PASS = range(4)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "frame_plan_check.cpp")])

    def ask(cases, rules="frame"):
        lines = [rules + " %d %d %d %d %d %d %d %d" % c for c in cases]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [_parse(a) for a in answers]
    return ask


def _parse(line):
    code, message, outputs, passes, path, extra = line.split("|")
    return dict(code=int(code), message=message,
                outputs=[tuple(int(v) for v in o.split(":")) for o in outputs.split(",") if o],
                passes=[int(v) for v in passes.split(",") if v], path=int(path), extra=int(extra))


def _error(code, message):
    return dict(code=code, message=message, outputs=[], passes=[], path=0, extra=0)


# ------------------------------------------------------------------ the rules, restated
def restate(beauty, bits, moment, adaptive, K, matte, n_ids, integrator):
    """A whole frame's plan.  bits: 1 albedo, 2 normal; K: cascade layers (0: none); matte: on / off."""
    if moment and not beauty:
        return _error(E_INVALID, "the moment image needs the path kernel: it cannot be rendered without the beauty")
    if K and (not beauty or adaptive):
        return _error(E_UNSUPPORTED, "the cascade layers need the beauty and a uniform render")
    if matte and (K or adaptive):
        return _error(E_UNSUPPORTED, "the matte planes need a uniform render without the cascade")
    if (bits or matte) and integrator == VOLUME:
        return _error(E_UNSUPPORTED, "first-hit AOVs need surfaces: the volume integrator has none")
    planes = -(-n_ids // 4) if matte else 0
    outputs = [(kind, 0) for kind, on in ((BEAUTY, beauty), (ALBEDO, bits & 1), (NORMAL, bits & 2), (MOMENT, moment)) if on]
    outputs += [(LAYER, j) for j in range(K)] + [(PLANE, q) for q in range(planes)]
    # cascade (reads Li_alpha first), moment (squares it in place; every adaptive level runs it for the
    # error estimate), then the two that overwrite it from the camera-ray hits
    passes = [name for name, on in ((CASCADE_PASS, K), (MOMENT_PASS, moment or adaptive), (FIRST_HIT_PASS, bits),
                                    (MATTE_PASS, planes)) if on]
    return dict(code=0, message="", outputs=outputs, passes=passes, path=int(bool(beauty)), extra=16 if K else 0)


MATTES = [(0, 0)] + [(1, n) for n in (0, 1, 4, 5, 32)]
CASES = [(beauty, bits, moment, adaptive, K, matte, n_ids, integrator)
         for beauty, bits, moment, adaptive, K, (matte, n_ids), integrator in
         itertools.product((0, 1), (0, 1, 2, 3), (0, 1), (0, 1), (0, 2, 8), MATTES, (PATH, VOLUME))]


def test_plan_frame_matches_the_rules(checker):
    assert len(CASES) == 1152
    seen = set()
    for c, got in zip(CASES, checker(CASES)):
        want = restate(*c)
        assert got == want, (c, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        beauty, bits, moment, adaptive, K, matte, n_ids, _ = c
        if got["code"] == 0:
            # neither an AOV-only nor a matte-only request launches the path kernel
            assert got["path"] == beauty
            assert len(got["outputs"]) <= 12 and len(set(got["outputs"])) == len(got["outputs"])
            assert got["outputs"] == sorted(got["outputs"])  # delivery order: kinds ascending, then indices
        seen.add((got["code"], got["message"]))
    assert len(seen) == 5 and {code for code, _ in seen} == {0, E_INVALID, E_UNSUPPORTED}  # every rule is reached


def test_first_broken_rule_wins(checker):
    """Requests that break several rules at once: today's precedence (moment, cascade, mattes, surfaces)."""
    both = checker([(0, 1, 1, 1, 2, 1, 4, VOLUME), (0, 1, 0, 1, 2, 1, 4, VOLUME), (1, 1, 0, 1, 0, 1, 4, VOLUME)])
    for b, start in zip(both, ("the moment image needs", "the cascade layers need", "the matte planes need")):
        assert b["message"].startswith(start), b
    assert [b["code"] for b in both] == [E_INVALID, E_UNSUPPORTED, E_UNSUPPORTED]


def test_spot_checks(checker):
    five, none, eight, no_beauty, cas_adaptive, aov_only, matte_only = checker([
        (1, 0, 0, 0, 0, 1, 5, PATH), (1, 0, 0, 0, 0, 1, 0, PATH), (1, 0, 0, 0, 8, 0, 0, PATH),
        (0, 0, 1, 0, 0, 0, 0, PATH), (1, 0, 0, 1, 2, 0, 0, PATH), (0, 3, 0, 0, 0, 0, 0, PATH), (0, 0, 0, 0, 0, 1, 4, PATH)])
    assert five["outputs"] == [(BEAUTY, 0), (PLANE, 0), (PLANE, 1)] and five["passes"] == [MATTE_PASS]
    assert none["outputs"] == [(BEAUTY, 0)] and none["passes"] == [] and none["code"] == 0
    assert len(eight["outputs"]) == 9 and eight["outputs"][1:] == [(LAYER, j) for j in range(8)]
    assert eight["passes"] == [CASCADE_PASS] and eight["extra"] == 16
    assert no_beauty["code"] == E_INVALID and cas_adaptive["code"] == E_UNSUPPORTED
    assert aov_only["path"] == 0 and aov_only["outputs"] == [(ALBEDO, 0), (NORMAL, 0)] and aov_only["passes"] == [FIRST_HIT_PASS]
    assert matte_only["path"] == 0 and matte_only["outputs"] == [(PLANE, 0)] and matte_only["passes"] == [MATTE_PASS]


def test_bucket_list_rules(checker):
    """A bare bucket-list render (an adaptive level, the asynchronous entry point) has two rules of its
    own, both NART_E_INVALID, and is not told about frames: an adaptive level is a uniform render of the
    beauty, the wanted AOVs and the moment tiles."""
    moment, cascade, level, too_many = checker([(0, 0, 1, 0, 0, 0, 0, PATH), (0, 0, 0, 0, 2, 0, 0, PATH),
                                                (1, 2, 1, 0, 0, 0, 0, PATH), (1, 0, 0, 0, 0, 1, 33, PATH)], rules="buckets")
    assert moment == _error(E_INVALID, "the moment image needs the path kernel (the beauty)")
    assert cascade == _error(E_INVALID, "the cascade layers need the path kernel (the beauty)")
    assert level["outputs"] == [(BEAUTY, 0), (NORMAL, 0), (MOMENT, 0)] and level["passes"] == [MOMENT_PASS, FIRST_HIT_PASS]
    assert too_many == _error(E_UNSUPPORTED, "the scene has 33 matte ids; at most 32 are supported")
