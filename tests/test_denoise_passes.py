"""The launch sequence, the work layout and the event budget of the three a-trous denoisers
(csrc/host/denoise_passes.h), checked on the CPU: what the driver of image_stages.h and the kernels rely
on, for 1..8 iterations with and without the variance kernel, and for every chunk plan of the parts."""
import os
import shutil
import subprocess
from collections import namedtuple

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ITERATIONS = list(range(1, 9))
HALO = [2, 4, 0, 0, 0, 0, 0, 0]
Launch = namedtuple("Launch", "kind halo slot src dst chunk step")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("denoise_passes") / "denoise_passes_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "native", "denoise_passes_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split("|") for a in answers]
    return ask


def _sequences(checker, lines):
    out = []
    for n, launches in checker(lines):
        seq = []
        for item in launches.split():
            kind, *nums = item.split(":")
            seq.append(Launch(kind, *[int(v) for v in nums]))
        assert len(seq) == int(n)
        out.append(seq)
    return out


def _limits(checker):
    ((limits,),) = checker(["limits"])
    return dict(zip(("iterations", "slots", "launches", "events"), (int(v) for v in limits.split())))


def _check_filter(seq, iterations, variance, chunk):
    """seq: the launches after prepare for one set of signals; returns nothing, asserts everything."""
    assert len(seq) == variance + iterations + 1
    kinds = [l.kind for l in seq]
    assert kinds == ["variance"] * variance + ["atrous"] * iterations + ["finalize"]
    assert all(l.chunk == chunk for l in seq)
    if variance:
        assert (seq[0].halo, seq[0].slot, seq[0].step) == (3, 1, 1)
    for i, l in enumerate(seq[variance:-1]):
        assert (l.step, l.halo, l.slot) == (2 ** i, HALO[i], 2 + i), (i, l)
    assert (seq[-1].slot, seq[-1].dst) == (10, -1)
    assert seq[-1].src == seq[-2].dst  # finalize reads what the last pass wrote
    for l in seq:
        assert l.src in (0, 1) and l.src != l.dst


@pytest.mark.parametrize("variance", [True, False])
def test_one_denoise(checker, variance):
    limits = _limits(checker)
    assert limits["iterations"] == 8 and limits["slots"] == 12
    for it, seq in zip(ITERATIONS, _sequences(checker, ["passes %d %d" % (it, variance) for it in ITERATIONS])):
        assert len(seq) == 2 + variance + it and len(seq) + 1 <= limits["events"]
        prepare = seq[0]
        assert (prepare.kind, prepare.slot, prepare.src, prepare.halo) == ("prepare", 0, -1, 0)
        assert ("variance" in [l.kind for l in seq]) == variance
        _check_filter(seq[1:], it, variance, 0)
        # every launch after prepare reads the buffer the launch before it wrote
        for before, after in zip(seq, seq[1:]):
            assert after.src == before.dst, (it, before, after)
        # the slots of the passes that do not run are never used, nor the sum's
        used = {l.slot for l in seq}
        assert used == {0, 10} | ({1} if variance else set()) | {2 + i for i in range(it)}
    assert _sequences(checker, ["passes 0 1", "passes 9 1", "passes 9 0"]) == [[], [], []]


def test_parts_denoise_and_the_event_budget(checker):
    limits = _limits(checker)
    cases = [(K, knob, it, s) for K in range(1, 10) for knob in range(5) for it in ITERATIONS for s in (0, 1)]
    seqs = _sequences(checker, ["parts %d %d %d %d" % c for c in cases])
    most = 0
    for (K, knob, it, s), seq in zip(cases, seqs):
        assert seq[0].kind == "prepare" and (seq[0].slot, seq[0].src, seq[0].dst) == (0, -1, 0)
        body = seq[1:-1] if s else seq[1:]
        if s:
            assert (seq[-1].kind, seq[-1].slot, seq[-1].src, seq[-1].dst) == ("sum", 11, -1, -1)
        assert "sum" not in [l.kind for l in body]
        per_chunk = it + 2
        assert len(body) % per_chunk == 0
        n_chunks = len(body) // per_chunk
        assert -(-K // 4) <= n_chunks <= K
        if knob:  # the chunks are the chunk plan's (test_denoise_parts_plan.py)
            assert n_chunks == -(-K // knob)
        for j in range(n_chunks):
            chunk = body[j * per_chunk:(j + 1) * per_chunk]
            _check_filter(chunk, it, True, j)
            assert chunk[0].src == seq[0].dst  # each chunk's variance reads what prepare wrote
            for before, after in zip(chunk, chunk[1:]):
                assert after.src == before.dst
        # the events the driver records: one before the first launch, one after each
        assert len(seq) <= limits["launches"] and len(seq) + 1 <= limits["events"]
        if (K, knob, it, s) == (9, 1, 8, 1):
            assert n_chunks == 9 and len(seq) + 1 == limits["events"]  # the budget is exact
        most = max(most, len(seq) + 1)
    assert most == limits["events"] == limits["launches"] + 1
    assert _sequences(checker, ["parts 0 0 5 1", "parts 10 0 5 1", "parts 3 0 0 1", "parts 3 0 9 1"]) == [[], [], [], []]


def test_work_layout(checker):
    npxs = [1, 3, 15, 70 * 3, 37 * 29, 129 * 65, 1920 * 1080]
    families = [("plain", 72, 1, 0), ("cross", 104, 2, 0)] + [("parts %d" % K, 40 + 36 * K, K, K) for K in range(1, 10)]
    for family, bpp, n_sig, n_alpha in families:
        for npx, (got_bpp, total, planes, named4, named1) in zip(npxs, checker(["work %s %d" % (family, npx) for npx in npxs])):
            assert int(got_bpp) == bpp, family
            assert int(total) == bpp * npx
            spans = [tuple(int(v) for v in p.split(":")) for p in planes.split()]
            assert len(spans) == (2 + 2 * n_sig) + (2 + n_alpha)
            # disjoint, inside the buffer, without gaps; the float4 planes first and 16-byte aligned
            at = 0
            for k, (off, size, elem) in enumerate(spans):
                assert off == at and off % elem == 0, (family, npx, k)
                assert elem == (16 if k < 2 + 2 * n_sig else 4) and size == elem * npx
                at += size
            assert at == int(total)
            # every named plane is a plane of its group, and no two names share one
            n4 = [int(v) for v in named4.split()]
            n1 = [int(v) for v in named1.split()]
            assert sorted(n4) == list(range(2 + 2 * n_sig)) and sorted(n1) == list(range(2 + n_alpha)), (family, n4, n1)
