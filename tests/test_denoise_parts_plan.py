"""The chunk plan of the parts denoise (csrc/host/denoise_parts_plan.h), checked on the CPU: what the
launches of image_stages.h rely on, for K = 1..9 and the knob NART_DN_PARTS_CHUNK at 0..4."""
import os
import re

import pytest

import denoise_parts_native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = list(range(1, 10))
KNOBS = [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return denoise_parts_native.build_checker(tmp_path_factory.mktemp("denoise_parts_plan"))


def _plans(checker, cases):
    out = []
    for (n, chunks) in checker(["plan %d %d" % c for c in cases]):
        ch = [tuple(int(v) for v in c.split(":")) for c in chunks.split()]
        assert len(ch) == int(n)
        out.append(ch)
    return out


def test_limits_agree(checker):
    ((limits,),) = checker(["max"])
    assert limits.split() == ["9", "9", "4"]
    header = open(os.path.join(REPO, "include", "nart_hip.h")).read()
    assert "#define NART_DENOISE_PARTS_MAX 9u" in header
    device = open(os.path.join(REPO, "nart_amd", "csrc", "device", "denoise_parts.h")).read()
    assert re.search(r"DNP_MAX_PARTS = 9;", device) and re.search(r"DNP_MAX_CHUNK = 4;", device)


def test_every_plan_partitions_the_parts(checker):
    cases = [(K, knob) for K in KS for knob in KNOBS]
    for (K, knob), chunks in zip(cases, _plans(checker, cases)):
        sizes = [s for _f, s in chunks]
        assert sum(sizes) == K, (K, knob, chunks)
        assert all(1 <= s <= 4 for s in sizes), (K, knob, chunks)
        # ascending, without gaps: chunk j starts where chunk j - 1 ended
        at = 0
        for first, size in chunks:
            assert first == at, (K, knob, chunks)
            at += size
        if knob:  # a forced size is honoured: every chunk has it, but one ragged last chunk
            assert sizes[:-1] == [knob] * (len(sizes) - 1) and 1 <= sizes[-1] <= knob, (K, knob, chunks)
            assert len(sizes) == -(-K // knob)


def test_the_automatic_plan_is_one_of_the_forced_ones(checker):
    """0 and anything out of range mean automatic; the automatic plan for K is the plan of one forced
    size (the measured one: the table in denoise_parts_plan.h)."""
    for K in KS:
        auto, big, *forced = _plans(checker, [(K, 0), (K, 5)] + [(K, c) for c in (1, 2, 3, 4)])
        assert auto == big and auto in forced, (K, auto)
    assert _plans(checker, [(0, 0), (10, 0), (10, 2)]) == [[], [], []]
