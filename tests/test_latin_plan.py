"""Which form of the LatinSquare a batch runs, where the three-kernel form's scratch arrays lie and how the
kernels are launched (csrc/host/latin_plan.h plan_latin), checked on the CPU against a restatement of
DESIGN.md section 4 (`k_latin_*`) and against what the kernels read, taken from device/kernels.h:

  k_latin_perm<BL>  a lane's choice words c[r * 64], rows r of its 64-slot group: PF = 16 rows before the first
                    swap and PF rows ahead of every full batch, unconditionally, so rows < n2 + PF.  LDS: a u16
                    column of 2 * n2 indices per lane of the block.
  k_latin_emit      16 slots per block of 256; index words of rows j0 + u * 16 (j0 < 16, u < U = 8) first, then
                    U * 16 rows ahead of the row it emits, unconditionally: rows < n2 + 2 * U * 16.  The
                    block's 16 * spp states are staged by 256 lanes x 8 loads of 16 B per round, unguarded:
                    up to 256 * 8 * 4 words past them.  LDS: the 16 * spp states.
  k_latin_lds       64 lanes, two float columns of spp per lane in LDS.
  k_latin_idx       64 lanes, u16 index columns of spp per lane: two up to 512 spp, one beyond; 2 * spp floats
                    of scratch per lane of every launched block.
"""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CU_LDS = 160 * 1024  # LDS of a gfx950 compute unit
THREE, LDS, IDX, GLOBAL = range(4)
SPPS = (1, 2, 64, 65, 256, 257, 512, 640, 642, 1024, 1025)
SLOTS = (1, 63, 64, 65, 192, 4096)
PF, EMIT_U, EMIT_SLOTS = 16, 8, 16


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("latin_plan") / "latin_plan_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "latin_plan_check.cpp")])

    def ask(cases):
        out = subprocess.run([exe], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = [{k: int(v) for k, v in (f.split("=") for f in line.split())} for line in out.stdout.splitlines()]
        assert len(answers) == len(cases)
        return answers
    return ask


def scratch_bytes(n_slots, spp):
    """The three-kernel form's scratch: four arrays of u16 pairs, a word per two samples and slot of every
    64-slot group, each with the rows the kernels read ahead; a state word per sample and slot of every
    16-slot block, with the words the staging reads past them."""
    n2, groups, blocks = -(-spp // 2), -(-n_slots // 64), -(-n_slots // EMIT_SLOTS)
    words = groups * 64 * n2 + 64 * max(PF, 2 * EMIT_U * 16)
    stw = blocks * EMIT_SLOTS * spp + 256 * 8 * 4
    return words, stw, 4 * (4 * words + stw)


def restate_form(n_slots, spp, capacity):
    if 64 < spp <= 1024 and scratch_bytes(n_slots, spp)[2] <= capacity:
        return THREE
    if spp <= 256:
        return LDS
    return IDX if spp <= 1024 and n_slots >= 64 else GLOBAL


def _cases():
    for n, spp in itertools.product(SLOTS, SPPS):
        need = scratch_bytes(n, spp)[2]
        # just below and just above what the three-kernel form needs; what ensure() gives a batch
        for cap in (need - 1, need, 16 * n * spp):
            yield n, spp, cap


def test_plan_latin_matches_the_policy_and_the_kernels_reads(checker):
    cases = list(_cases())
    forms, perm_blocks = set(), set()
    for (n, spp, cap), p in zip(cases, checker(cases)):
        c = (n, spp, cap)
        n2, groups = -(-spp // 2), -(-n // 64)
        assert p["form"] == restate_form(n, spp, cap), (c, p)
        assert p["n2"] == n2
        forms.add(p["form"])
        if p["form"] == THREE:
            words, stw, need = scratch_bytes(n, spp)
            # the arrays cover their rows and the read-ahead, lie apart in order and end within the buffer
            assert p["words"] >= groups * 64 * n2 + 64 * max(PF, 2 * EMIT_U * 16), (c, p)
            assert p["stw"] >= -(-n // EMIT_SLOTS) * EMIT_SLOTS * spp + 256 * 8 * 4, (c, p)
            assert (p["words"], p["stw"]) == (words, stw)
            starts = [p[k] for k in ("cx", "cy", "sx", "sy", "st")]
            assert starts[0] == 0 and all(b - a >= p["words"] for a, b in zip(starts, starts[1:])), (c, p)
            assert 4 * (p["st"] + p["stw"]) <= cap, (c, p)
            # 80-lane blocks exactly where a 64-lane block's columns leave no room for a second one on the CU
            bl = p["perm_block"]
            assert bl == (80 if n2 * 4 * 128 > CU_LDS else 64), (c, p)
            perm_blocks.add(bl)
            assert (p["draws_threads"], p["draws_lds"]) == (256, 0) and p["draws_blocks"] * 256 >= n > (p["draws_blocks"] - 1) * 256
            assert p["perm_threads"] == bl and p["perm_blocks"] * bl >= n > (p["perm_blocks"] - 1) * bl, (c, p)
            assert p["perm_lds"] == 2 * n2 * bl * 2 <= CU_LDS, (c, p)
            assert p["emit_threads"] == 256 and p["emit_blocks"] * EMIT_SLOTS >= n > (p["emit_blocks"] - 1) * EMIT_SLOTS
            assert p["emit_lds"] == 4 * EMIT_SLOTS * spp <= CU_LDS, (c, p)
        else:
            per = 256 if p["form"] == GLOBAL else 64
            assert p["one_threads"] == per and p["one_blocks"] * per >= n > (p["one_blocks"] - 1) * per, (c, p)
            lds = {LDS: 2 * 4 * 64 * spp, IDX: (2 if spp <= 512 else 1) * 2 * 64 * spp, GLOBAL: 0}[p["form"]]
            assert p["one_lds"] == lds <= CU_LDS, (c, p)
            if p["form"] == IDX and cap >= 16 * n * spp:
                assert p["one_blocks"] * 64 * 2 * spp * 4 <= cap, (c, p)  # its value scratch fits the record buffer
    assert forms == {THREE, LDS, IDX, GLOBAL} and perm_blocks == {64, 80}


def test_plan_latin_of_known_batches(checker):
    """The forms the measurement notes and the GPU tests count on, each batch with the record buffer ensure()
    gives it (16 B per sample): a C3 batch (256 spp) runs the three kernels with 64-lane blocks; a 16x12
    rectangle at 1,024 spp runs them with 80-lane blocks; a single bucket at 256 spp is too small for the
    scratch's padding and keeps k_latin_lds."""
    def ask(n, spp):
        p = checker([(n, spp, 16 * n * spp)])[0]
        return p["form"], p["perm_block"]

    assert ask(8160 * 256, 256) == (THREE, 64)
    assert ask(16 * 12, 1024) == (THREE, 80)
    assert ask(16 * 12, 642) == (THREE, 80)
    assert ask(16 * 12, 640) == (THREE, 64)
    assert ask(256, 256)[0] == LDS
    assert ask(256, 64)[0] == LDS
    assert ask(16 * 12, 1025)[0] == GLOBAL
