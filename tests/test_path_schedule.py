"""The path kernels' launch schedule (csrc/host/path_schedule.h plan_path) and the layout of the
probe-ordered pixel queue (csrc/device/queue_layout.h queue_entry), checked on the CPU.

plan_path is compared, field by field, with a restatement of the policy as DESIGN.md section 4
("Scheduling") and the measurement notes describe it, over a grid of launches that crosses every
threshold from both sides with each knob set as the GPU tests set it.  queue_entry is checked
against the properties the ray-queue kernel relies on: every pixel queued, the costly ones on
adjacent aligned lanes of one first-round wave, the flag bits telling which is which."""
import itertools
import os
import shutil
import subprocess

import pytest

from nart_amd.api import SCHED

HERE = os.path.dirname(os.path.abspath(__file__))
KNOBS = ["NART_PRIMARY_PACKET", "NART_RQ_PRIO", "NART_RQ_PAIRS", "NART_RQ_HALF", "NART_RQ_QUAD", "NART_RQ_SETPRIO",
         "NART_RQ_ORDER", "NART_RQ_TOPF", "NART_PROBE_SUB", "NART_QUEUE_K"]
DIRECT, GROUPS, PIXEL_QUEUE, WHOLE_GROUPS = range(4)
NO_PROBE, EVERY_PIXEL, SAMPLED = range(3)
PRIO_BIT, PAIR_BIT, QUAD_BIT = 0x80000000, 0x40000000, 0x20000000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("path_schedule") / "path_schedule_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "path_schedule_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


# ------------------------------------------------------------------ the policy, restated
def restate(n, res_k, res_rq, rq_block, wv, pr, env, rq, spec, has_prim, kn):
    """The schedule of a launch of n traced pixels.  res_k / res_rq: resident 256-lane blocks of
    k_render / of the ray-queue kernel; kn: {knob: text} of the knobs that are set."""
    def num(name, default):
        return float(kn[name]) if kn.get(name) else default

    s = dict(error=0, shape=DIRECT, primary=0, packet=int(num("NART_PRIMARY_PACKET", 1) != 0), queue_room=0,
             probe=NO_PROBE, probe_sub=64, probe_blocks=0, order=0, E=0, k=0, pairs=0, half=0, quad=0, rq_prio=0,
             rq_setprio=0, qlen=0, qbase=0)
    names = set()
    if rq and spec:
        names.add("specialized")
    if rq and wv == 3 and not pr:
        names.add("lean")
    if rq and has_prim:  # camera rays first, for the ray-queue kernel only
        s["primary"] = 1
        names.add("primary")
    # every threshold counts rounds of k_render's resident waves; the grid and the first round's
    # waves are those of the kernel that runs
    rounds = n / (256.0 * res_k)
    resident = res_rq if rq else res_k
    waves = 4 * resident
    all_blocks = -(-n // 256)
    groups_of_64 = -(-n // 64)
    s.update(resident=resident, W=waves, blocks=all_blocks)
    s["rq_quorum"] = 8 if rounds >= 3 else 0  # throughput-bound launches leave a traversal phase early

    def done():
        s["sched"] = sum(SCHED[x] for x in names)
        return s

    if all_blocks <= resident:
        return done()  # a resident lane for every pixel: nothing to schedule
    s["queue_room"] = n + 63 * waves

    # many rounds: slot order.  k_render launches it as it is (from 12 rounds); the ray-queue kernel
    # takes 64-slot groups on a persistent grid from 6 rounds, its lean build from 3.  NART_QUEUE_K
    # asks for the pixel queue whatever the size.
    many = (3 if wv == 3 else 6) if rq else 12
    if rounds >= many and "NART_QUEUE_K" not in kn:
        if not rq:
            return done()
        s["shape"] = GROUPS
        names.add("wave_groups")
        s["blocks"] = min(all_blocks, resident)
        order = int(num("NART_RQ_ORDER", 2 if env else 1))
        if order in (1, 2):  # costliest groups first needs a probe; slot order (anything else) none
            s["order"] = order
            sub = int(num("NART_PROBE_SUB", 8 if rounds >= 12 else 64))
            if sub not in (1, 2, 4, 8, 16, 32):
                sub = 64
            s["probe_sub"] = sub
            s["probe"] = SAMPLED if sub < 64 else EVERY_PIXEL
            s["probe_blocks"] = -(-groups_of_64 * sub // 256) if sub < 64 else all_blocks
            if order == 2:
                share = max(0.0, num("NART_RQ_TOPF", 10)) * 0.01 * groups_of_64
                s["E"] = int(min(float(groups_of_64), share))
        return done()

    # the probe-ordered pixel queue
    s["probe"], s["probe_blocks"] = EVERY_PIXEL, all_blocks
    # priority lanes: the ray-queue builds that have them, on shards below 3 rounds (2: always, 0: never)
    want = int(num("NART_RQ_PRIO", 1))
    prio = rq and pr and (want == 2 or (want == 1 and rounds < 3))
    lanes = int(num("NART_RQ_PAIRS", 2))
    lanes = 0 if lanes <= 0 else (4 if lanes >= 4 else 2)
    block_waves = rq_block // 64
    per_simd = block_waves // 4

    def fits_half(k, group):  # the costly pixels of a block's waves on its first four
        return per_simd * max(group, 1) * k <= 64

    k_half = 12 if per_simd == 2 else 8
    half = bool(prio and num("NART_RQ_HALF", 1) != 0 and waves % block_waves == 0 and rounds < 3 and
                fits_half(k_half, lanes if lanes * k_half <= 64 else 0))
    k = 32 if rounds >= 3 else (k_half if half else 8)
    if "NART_QUEUE_K" in kn:
        k = int(max(1.0, min(64.0, num("NART_QUEUE_K", 8))))
    s["k"] = k
    if k == 64:
        s["shape"] = WHOLE_GROUPS
        return done()
    s["shape"] = PIXEL_QUEUE
    names.add("probe_queue")
    group = lanes if prio and lanes * k <= 64 else 0
    half = half and fits_half(k, group)
    quad = bool(prio and group == 2 and 2 * k + 2 <= 64 and num("NART_RQ_QUAD", 0) != 0)
    s.update(pairs=group, quad=int(quad), half=block_waves if half and not quad else 0, rq_prio=int(prio))
    s["qlen"] = n + (group - 1) * k * waves * (group > 0) + 2 * waves * quad
    if prio:
        names.add("priority")
        s["rq_setprio"] = int(max(0.0, num("NART_RQ_SETPRIO", 1 if half else 0)))
    if group:
        names.add("spec_pairs")
    if s["half"]:
        names.add("half_waves")
    unit = rq_block // 256 if rq else 1  # whole blocks of the kernel that runs
    s["blocks"] = -(-resident // unit) * unit
    s["qbase"] = 256 * s["blocks"]
    return done()


KNOB_SETTINGS = [{}] + [{k: v} for k, vs in [("NART_RQ_PRIO", "012"), ("NART_RQ_PAIRS", "024"), ("NART_RQ_HALF", "0"),
                                             ("NART_RQ_QUAD", "1"), ("NART_RQ_SETPRIO", "0"),
                                             ("NART_PRIMARY_PACKET", "0")] for v in vs] + \
    [{"NART_RQ_ORDER": o, "NART_RQ_TOPF": "15"} for o in "012"] + \
    [{"NART_PROBE_SUB": v} for v in ("1", "8", "64")] + [{"NART_QUEUE_K": v} for v in ("1", "8", "64")] + \
    [{"NART_RQ_PRIO": "2", "NART_RQ_PAIRS": "4"}, {"NART_RQ_PRIO": "2", "NART_RQ_QUAD": "1"},
     {"NART_RQ_PRIO": "2", "NART_QUEUE_K": "31", "NART_RQ_QUAD": "1"}, {"NART_QUEUE_K": "16", "NART_RQ_PAIRS": "4"},
     {"NART_QUEUE_K": "20", "NART_RQ_PAIRS": "4"}]


def _launches():
    for res_k in (1, 6, 256, 512):
        lanes = 256 * res_k
        sizes = {lanes, lanes + 1, 2 * lanes, 2 * lanes + 1}  # blocks <= / > resident, either kernel
        for t in (1.0, 1.5, 3.0, 6.0, 12.0):  # rounds just below, at and above each threshold
            m = int(t * lanes)
            sizes |= {m - 1, m, m + 37, m + 100}
        sizes |= {3 * lanes + 64, 14 * lanes + 7}
        for wv, pr, env, rq in itertools.product((2, 3), (1, 0), (0, 1), (1, 0)):
            rq_block = 768 if wv == 3 else 512
            cus = max(1, res_k // 2)  # one ray-queue block per CU, two k_render blocks
            yield from ((n, res_k, cus * rq_block // 256, rq_block, wv, pr, env, rq) for n in sorted(sizes))
    # the first round's waves are no whole number of ray-queue blocks: no half layout, k = 8 dealt
    # over every wave
    for n in (3 * 256 + 1, 5 * 256 + 100, 10 * 256):
        yield (n, 3, 3, 512, 2, 1, 0, 1)
        yield (n, 2, 5, 768, 3, 1, 0, 1)
    # the counting build's 256-lane ray-queue blocks
    for n in (257, 600, 2000, 4000):
        yield (n, 1, 1, 256, 2, 1, 0, 1)


def test_plan_path_matches_the_policy(checker):
    cases = [(c, kn) for c in _launches() for kn in KNOB_SETTINGS]
    lines = ["plan %d %d %d %d %d %d %d %d %d %d " % (c + (c[7], 1)) + " ".join(kn.get(k, "-") for k in KNOBS)
             for c, kn in cases]
    seen = set()
    for (c, kn), line in zip(cases, checker(lines)):
        got = {k: int(v) for k, v in (f.split("=") for f in line.split())}
        want = restate(*c, spec=c[7], has_prim=1, kn=kn)
        assert got == want, (c, kn, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        assert got["qlen"] <= got["queue_room"] or got["shape"] != PIXEL_QUEUE  # ensure_queue's size
        assert got["error"] == 0
        seen.add((got["shape"], got["probe"], got["order"], bool(got["half"]), got["pairs"], got["quad"], got["k"]))
    # the grid reaches every path
    assert {s[0] for s in seen} == {DIRECT, GROUPS, PIXEL_QUEUE, WHOLE_GROUPS}
    assert {s[1] for s in seen} == {NO_PROBE, EVERY_PIXEL, SAMPLED} and {s[2] for s in seen} == {0, 1, 2}
    assert {s[4] for s in seen} == {0, 2, 4} and {s[5] for s in seen} == {0, 1}
    assert {s[6] for s in seen if s[0] == PIXEL_QUEUE} >= {1, 8, 12, 16, 20, 31, 32}
    assert {s[3] for s in seen} == {False, True}


def test_half_layout_falls_back_when_waves_do_not_fill_blocks(checker):
    """W % BW != 0: no half waves, k = 8 dealt over every wave, pairs kept."""
    line, = checker(["plan 869 3 3 512 2 1 0 1 1 1 " + " ".join("-" * len(KNOBS))])
    got = {k: int(v) for k, v in (f.split("=") for f in line.split())}
    assert (got["W"], got["k"], got["half"], got["pairs"], got["shape"]) == (12, 8, 0, 2, PIXEL_QUEUE)
    assert got["sched"] & SCHED["half_waves"] == 0 and got["sched"] & SCHED["priority"]


# ------------------------------------------------------------------ the queue layout
LAYOUTS = [(8, 0, 0, 0), (8, 2, 0, 0), (8, 4, 0, 0), (16, 4, 0, 0), (32, 2, 0, 0), (12, 2, 8, 0), (12, 0, 8, 0),
           (8, 4, 8, 0), (8, 2, 12, 0), (8, 2, 0, 1), (31, 2, 0, 1)]


def test_queue_layout(checker):
    cases = [(n, W, k, PRIO_BIT, pairs, half, quad) for W in (24, 48) for n in (64 * W + 1, 64 * W + 100, 128 * W + 37)
             for k, pairs, half, quad in LAYOUTS]
    for (n, W, k, prio, pairs, half, quad), line in zip(cases, checker(["queue %d %d %d %d %d %d %d" % c for c in cases])):
        v = [int(x) for x in line.split()]
        per = max(pairs, 1)
        assert v[0] == n + (per - 1) * k * W + (2 * W if quad else 0) == (len(v) - 1) // 3
        entries = list(zip(v[1::3], v[2::3], v[3::3]))
        rest = [i for top, i, _ in entries if not top]
        assert sorted(rest) == list(range(n - k * W))  # every other pixel exactly once
        where = {}
        for p, (top, i, flags) in enumerate(entries):
            if top:
                where.setdefault(i, []).append(p)
            else:
                assert flags == 0
        assert sorted(where) == list(range(k * W))  # every costly pixel
        for i, ps in where.items():
            copies = 4 if quad and i < W else per
            assert ps == list(range(ps[0], ps[0] + copies)), (i, ps)  # adjacent lanes ...
            assert ps[0] % copies == 0 and ps[-1] < 64 * W and ps[0] // 64 == ps[-1] // 64  # ... of one first-round wave
            if half:
                assert (ps[0] // 64) % half < 4  # on the block's first four waves (one per SIMD)
            want = prio | (PAIR_BIT if pairs else 0) | (QUAD_BIT if copies == 4 and quad else 0)
            assert all(entries[p][2] == want for p in ps), (i, hex(want))
        if not quad and not half:  # dealt round robin: wave w holds the ranks w, W + w, ...
            assert all(ps[0] // 64 == i % W for i, ps in where.items())
