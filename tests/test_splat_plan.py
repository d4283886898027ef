"""Which splat kernel a call runs and how a batch launches it (csrc/host/splat_plan.h plan_splat,
splat_launch, splat_scalars), checked on the CPU.

plan_splat is compared, field by field, with a restatement of the policy as DESIGN.md (section 4, the
`k_splat_skew` / `k_splat_rows` / `k_splat_col4` notes) and INTEGRATION.md (the splat-mode row) describe it,
over a grid that crosses every threshold from both sides with each knob set as the GPU tests set it.  Every
splat_launch is checked against what the kernel it names relies on, read off device/kernels.h:

  k_splat_rows<R>     `U = tile * (2R + 1)` lanes per bucket, `UB = blockDim.x / U` buckets per block, bucket
                      `blockIdx.x * UB + lb`; lanes with `lb >= UB` idle.  `__launch_bounds__(512)`.  Dynamic LDS:
                      `lut_n` float4 cells, then `s_flag[2 * UB]` words.  So the host's buckets per block must
                      equal blockDim.x / U (the flag words it reserved), and whole waves are launched.
  k_splat_skew<R, NB> 256 lanes = 4 waves; `PB = 64 / tile` units of `tile` lanes per wave; unit
                      `(blockIdx.x * 4 + wave) * PB + lb` is band `unit % NB` of bucket `unit / NB`.  Dynamic LDS:
                      `lut_n` float4 cells, then `s_flag[8 * PB]` words (two per unit of the block).
  k_splat_col4<NP>    256 lanes, static LDS only; lane `gid` serves rows `NP * (rem / tile) ..` of a tile column,
                      `gid < n_buckets * tile * ceil(tile / NP)`.
  k_splat<MODE>       256 lanes, static LDS only; one lane per tile pixel, `gid < n_buckets * tile * tile`.
"""
import itertools
import os
import shutil
import subprocess

import pytest

from nart_amd.api import SCHED

HERE = os.path.dirname(os.path.abspath(__file__))
CU_LDS = 160 * 1024  # LDS of a gfx950 compute unit
ROWS, SKEW, COL4, PIXEL = range(4)
NP = 4  # tile pixels per lane of k_splat_col4


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("splat_plan") / "splat_plan_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "splat_plan_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


def _fields(text):
    return {k: int(v) for k, v in (f.split("=") for f in text.split())}


# ------------------------------------------------------------------ the choice, restated
def waves_per_simd_x(tile, n_buckets):
    """Waves of a one-band k_splat_skew launch: floor(64 / tile) buckets share a wave; none when a tile
    column does not fit a wave."""
    return -(-n_buckets // (64 // tile)) if tile <= 64 else 0


def preconditions(B, fb, tile, lut_ok):
    """What the skewed kernels need: the filter-cell table, a power-of-two bucket of at most 32, a tile
    column within a wave, filter bounds 1..3 (their template argument)."""
    return [bool(lut_ok), B & (B - 1) == 0 and B <= 32, tile <= 64, 1 <= fb <= 3]


def restate_choice(mode, volume, B, fb, tile, n_buckets, n_cus, lut_ok, small, bands):
    waves, simds = waves_per_simd_x(tile, n_buckets), 4 * n_cus
    if mode < 0:
        # the default: k_splat_skew from 2 waves per SIMD (the volume integrator: from 1), below it
        # k_splat_rows, or k_splat_col4 with NART_SPLAT_SMALL=col4
        mode = 4 if waves >= (1 if volume else 2) * simds else (3 if small else 5)
    # one band per bucket from 2 waves per SIMD, else two; NART_SKEW_BANDS forces 1 or 2
    nb = (2 if int(float(bands)) >= 2 else 1) if bands and int(float(bands)) > 0 else (1 if waves >= 2 * simds else 2)
    skew = mode >= 4 and all(preconditions(B, fb, tile, lut_ok))
    return dict(mode=mode, skew=int(skew), rows=int(skew and mode == 5), bands=nb)


# (unset, or as tests/test_gpu_parity.py sets NART_SKEW_BANDS; NART_SPLAT_SMALL is the word col4 or not)
KNOBS = [(0, None), (0, "1"), (0, "2"), (1, None), (1, "2"), (0, ""), (0, "0")]
# the default mode with every knob; forced modes, which NART_SPLAT_SMALL does not reach, with the band knob
MODES_KNOBS = [(-1, k) for k in KNOBS] + [(m, KNOBS[0]) for m in (0, 1, 3, 4, 5)] + [(m, k) for m in (4, 5) for k in KNOBS[1:3]]


def _bucket_counts(tile, n_cus):
    """Bucket counts whose waves land one below, at and one above 1 and 2 waves per SIMD (the volume
    integrator's threshold, the path integrator's, which is also the band boundary); the wave count at a
    threshold from its smallest bucket count too."""
    per = 64 // tile if tile <= 64 else 1
    out = set()
    for t in (4 * n_cus, 8 * n_cus):
        out |= {(t - 1) * per, (t - 1) * per + 1, t * per, (t + 1) * per}
    return sorted(n for n in out if n > 0)


def _choice_cases():
    for n_cus, tile, B, fb, volume, lut_ok in itertools.product((1, 8, 256), (6, 18, 20, 36, 64, 65), (4, 12, 16, 32, 64),
                                                                (0, 1, 2, 3, 4), (0, 1), (0, 1)):
        for nb, (mode, (small, bands)) in itertools.product(_bucket_counts(tile, n_cus), MODES_KNOBS):
            yield (mode, volume, B, fb, tile, nb, n_cus, lut_ok, small), bands


def _choice_line(c, bands):
    return "choice %d %d %d %d %d %d %d %d %d " % c + {None: "-", "": "="}.get(bands, bands)


def test_plan_splat_matches_the_policy(checker):
    cases = list(_choice_cases())
    seen = set()
    for (c, bands), line in zip(cases, checker([_choice_line(c, bands) for c, bands in cases])):
        got, want = _fields(line), restate_choice(*c, bands)
        assert got == want, (c, bands, got, want)
        mode, volume, B, fb, tile, nb, n_cus, lut_ok, small = c
        waves = waves_per_simd_x(tile, nb)
        if mode < 0:
            # the default: 4 or 5 (3 with NART_SPLAT_SMALL=col4), on the right side of the threshold; the
            # volume integrator's threshold is half the path integrator's
            threshold = (4 if volume else 8) * n_cus
            assert got["mode"] == (4 if waves >= threshold else (3 if small else 5)), (c, got)
            seen.add((volume, got["mode"], waves - threshold))
        else:
            assert got["mode"] == mode
        ok = preconditions(B, fb, tile, lut_ok)
        assert got["skew"] == int(all(ok) and got["mode"] >= 4)
        assert not got["rows"] or got["skew"]
        assert got["bands"] in (1, 2)
    # the grid crosses both thresholds from both sides, with both small modes
    for volume in (0, 1):
        assert {(volume, 4, 0), (volume, 4, 1), (volume, 5, -1), (volume, 3, -1)} <= seen


def test_plan_splat_each_precondition_alone(checker):
    """skew is false when any one precondition fails, each failed alone from a cell where all hold."""
    good = dict(B=16, fb=2, tile=20, lut_ok=1)
    broken = [dict(lut_ok=0), dict(B=12), dict(B=64), dict(tile=65), dict(fb=0), dict(fb=4)]
    cases = [dict(good, **b) for b in [{}] + broken]
    for mode in (4, 5, -1):
        lines = [_choice_line((mode, 0, c["B"], c["fb"], c["tile"], 100000, 8, c["lut_ok"], 0), None) for c in cases]
        got = [_fields(a) for a in checker(lines)]
        assert got[0]["skew"] == 1 and got[0]["rows"] == int(mode == 5)
        for c, g in zip(cases[1:], got[1:]):
            assert sum(preconditions(c["B"], c["fb"], c["tile"], c["lut_ok"])) == 3  # exactly one fails
            assert g["skew"] == 0 and g["rows"] == 0, c


def test_plan_splat_benchmark_frames(checker):
    """The choices the measurement notes state for an MI355X (256 CUs), bucket 16, filter width 2 (tile 20,
    three buckets per wave): a 1920x1080 frame (8,160 buckets, 2,720 waves >= 2,048) runs k_splat_skew with
    one band; its 1/2 shard (1,360 waves) k_splat_rows, or for the volume integrator k_splat_skew with two
    bands; a 1/8 shard k_splat_rows for both."""
    def ask(volume, n):
        return _fields(checker([_choice_line((-1, volume, 16, 2, 20, n, 256, 1, 0), None)])[0])

    assert ask(0, 8160) == dict(mode=4, skew=1, rows=0, bands=1)
    assert ask(0, 4080) == dict(mode=5, skew=1, rows=1, bands=2)
    assert ask(1, 4080) == dict(mode=4, skew=1, rows=0, bands=2)
    assert ask(1, 1020) == dict(mode=5, skew=1, rows=1, bands=2)


# ------------------------------------------------------------------ the launch
def _launch_cases():
    tiles = sorted({B + 2 * fb for B in (4, 8, 16, 32) for fb in (1, 2, 3)} | {12 + 4, 64})
    for lut_cells, nbk, tile, fb in itertools.product((0, 700, 2048), (1, 2, 3, 4, 7, 25, 64, 65, 1000), tiles, (1, 2, 3)):
        for bands in (1, 2):
            yield (4, 1, 0, bands, fb, tile, 1, 1, lut_cells, nbk)  # k_splat_skew
        yield (5, 1, 1, 2, fb, tile, 1, 1, lut_cells, nbk)  # k_splat_rows
        for mode, thr_ok, invB_ok in itertools.product((0, 1, 3, 4, 5), (0, 1), (0, 1)):
            yield (mode, 0, 0, 1, fb, tile, thr_ok, invB_ok, lut_cells, nbk)  # the gather kernels


def _covers(blocks, per_block, units):
    """`blocks` blocks of per_block units serve `units`, and one block fewer would not."""
    return blocks * per_block >= units > (blocks - 1) * per_block


def test_splat_launch_is_what_the_kernels_rely_on(checker):
    cases = list(_launch_cases())
    kinds = set()
    for c, line in zip(cases, checker(["launch " + " ".join(map(str, c)) for c in cases])):
        mode, skew, rows, bands, fb, tile, thr_ok, invB_ok, lut_cells, nbk = c
        l = _fields(line)
        kinds.add(l["kernel"])
        assert l["lds"] <= CU_LDS and 1 <= l["threads"] <= 1024 and l["blocks"] >= 1, (c, l)
        if rows:
            U = tile * (2 * fb + 1)
            ub = l["per_block"]
            assert (l["kernel"], l["fb"], l["sched"]) == (ROWS, fb, SCHED["splat_rows"]), (c, l)
            assert _covers(l["blocks"], ub, nbk), (c, l)
            assert ub >= 1 and ub * U <= l["threads"] and l["threads"] % 64 == 0 and l["threads"] <= 512, (c, l)
            assert l["threads"] // U == ub, (c, l)  # the kernel's UB: the flag words reserved are the ones it clears
            assert l["lds"] == 16 * lut_cells + 4 * 2 * ub, (c, l)
        elif skew:
            pb = 64 // tile
            assert (l["kernel"], l["fb"], l["bands"], l["sched"]) == (SKEW, fb, bands, SCHED["splat_skew"]), (c, l)
            assert l["threads"] == 256 and pb >= 1 and l["per_block"] == 4 * pb, (c, l)
            assert _covers(l["blocks"], 4 * pb, nbk * bands), (c, l)
            assert l["lds"] == 16 * lut_cells + 4 * 8 * pb, (c, l)
        else:
            col4 = thr_ok and invB_ok and mode >= 3
            assert l["kernel"] == (COL4 if col4 else PIXEL) and l["sched"] == 0, (c, l)
            assert l["threads"] == 256 and l["lds"] == 0, (c, l)
            lanes = nbk * tile * (-(-tile // NP) if col4 else tile)
            assert _covers(l["blocks"], 256, lanes), (c, l)
            if col4:
                assert l["lut"] == int(lut_cells > 0), (c, l)
            else:
                assert l["thr"] == int(bool(thr_ok) and mode >= 1), (c, l)
    assert kinds == {ROWS, SKEW, COL4, PIXEL}


def test_splat_scalars(checker):
    """invB and invFw are the exact reciprocals of a power of two and 0 otherwise (the kernels then divide);
    idx_scale is 64 / fw in float."""
    import numpy as np
    cases = [(2.0, 16), (1.5, 12), (0.5, 32), (3.0, 4), (0.75, 24), (4.0, 1)]
    for (fw, B), line in zip(cases, checker(["scalars %r %d" % c for c in cases])):
        got = {k: float(v) for k, v in (f.split("=") for f in line.split())}
        pow2 = lambda v: v > 0 and np.frexp(v)[0] == 0.5
        assert got["invB"] == (1.0 / B if pow2(B) else 0.0)
        assert got["invFw"] == (1.0 / fw if pow2(fw) else 0.0)
        assert np.float32(got["idx_scale"]) == np.float32(64.0) / np.float32(fw)
