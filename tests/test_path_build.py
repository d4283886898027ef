"""Which build of the path kernels a launch runs and its LDS layout (csrc/host/path_build.h plan_build),
and the volume integrator's launch (csrc/host/path_schedule.h plan_volume, sparse_hot_groups), checked
on the CPU.

Each function is compared, field by field, with a restatement of the policy as DESIGN.md ("Build x
schedule coverage", section 4's scheduling and specialisation notes) and the measurement comments
describe it, over a grid that crosses every threshold from both sides with each knob set as the GPU
tests set it.  The cells of DESIGN.md's coverage table that read "cannot occur" are asserted over the
product of plan_build and plan_path (the launch stated as render.hip launch_render states it)."""
import itertools
import os
import shutil
import subprocess

import pytest

from nart_amd.api import FEATURES as FT, FT_ALL, SCHED

HERE = os.path.dirname(os.path.abspath(__file__))
CU_LDS = 160 * 1024  # LDS of a gfx950 compute unit
FM_DIFFUSE = FT["lambert"] | FT["disk"]
FM_GLASS = FT["lambert"] | FT["glass"] | FT["disk"]
FM_ENVTEX = FT["lambert"] | FT["plastic"] | FT["environment"] | FT["texture"] | FT["normal_map"]
OFF, ON, LEAN = range(3)  # nart_hip_set_specialize
DIRECT, GROUPS, PIXEL_QUEUE, WHOLE_GROUPS = range(4)
COUNTER, FOUR_WAVE, PLAIN = range(3)
RANGE_ERROR = "ray-queue LDS layout out of range"
# the instantiations render.hip's table holds: {ext, count, env, fm, wv, pr}
BUILDS = {(e, c, v, FT_ALL, 2, 1) for e in (0, 1) for c in (0, 1) for v in (0, 1)} | \
    {(0, 0, env, fm, wv, pr) for fm, env in ((FM_DIFFUSE, 0), (FM_GLASS, 0), (FM_ENVTEX, 1)) for wv, pr in ((2, 1), (3, 0))}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path_factory.mktemp("path_build") / "path_build_check")
    subprocess.check_call([hipcc, "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "native", "path_build_check.cpp")])

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return answers
    return ask


def _fields(text):
    return {k: float(v) if k == "f" else int(v) for k, v in (f.split("=") for f in text.split())}


def _knob(kn, name):
    return {None: "-", "": "="}.get(kn.get(name), kn.get(name))


def _num(kn, name, default):
    return float(kn[name]) if kn.get(name) else default


# ------------------------------------------------------------------ the build and its layout, restated
def rq_fixed_lds(levels, lanes):
    """What a ray-queue block keeps in LDS before the staged nodes: per lane 8 B per stack level and a
    16-B result; per wave the outbox (3 ray kinds x 64 lanes x 32 B) and two rings of 256 one-byte ids."""
    waves = lanes // 64
    return lanes * (8 * levels + 16) + waves * (3 * 64 * 32 + 2 * 256)


def staged(nodes, fixed, budget):
    """Top BVH nodes (64 B each) in what the fixed part leaves of the budget."""
    return min(nodes, max(0, budget - fixed) // 64)


def restate_build(features, env, spec, counters, bounces, variant, depth, nodes, n, res_k, kn):
    # k_render: 256 lanes, two blocks share a CU's LDS
    k_nodes = staged(nodes, 2048 * depth, CU_LDS // 2)
    s = dict(k_nodes=k_nodes, k_lds=2048 * depth + 64 * k_nodes, env=env)
    # the ray-queue kernel where variant 0 asks for it and the 512-lane layout fits a CU (or the lowered limit)
    rq = variant == 0 and rq_fixed_lds(depth, 512) <= int(min(_num(kn, "NART_RQ_LDS_LIMIT", CU_LDS), CU_LDS))
    fm = FT_ALL
    if spec != OFF and not counters and bounces <= 10:
        fm = next((m for m in ((FM_ENVTEX,) if env else (FM_DIFFUSE, FM_GLASS)) if features & ~m == 0), FT_ALL)
    generic = fm == FT_ALL
    # lean: throughput-bound launches of a specialised build; glass scenes from 12 rounds of k_render's
    # resident waves, environment-lit ones from 3, the others from 1.5
    first = 12.0 if features & FT["glass"] else (3.0 if env else 1.5)
    lean = not generic and spec == LEAN and rq and n / (256.0 * res_k) >= _num(kn, "NART_LEAN_ROUNDS", first)
    s.update(ext=int(generic and bounces > 10), count=int(generic and counters), fm=fm, wv=3 if lean else 2,
             pr=0 if lean else 1, rq=int(rq), fm_used=fm if rq else FT_ALL)
    lanes = 256 if s["count"] else (768 if lean else 512)
    levels = depth
    if lean and "NART_LEAN_STACK" in kn:
        levels = max(1, min(depth, int(_num(kn, "NART_LEAN_STACK", 1))))
    elif lean:
        # every level where 320 nodes (or the whole BVH) still fit beside them, else as many as do, 4 at least
        room = CU_LDS - 64 * min(nodes, 320) - rq_fixed_lds(0, 768)
        levels = min(depth, max(4, room // (8 * 768)))
    fixed = rq_fixed_lds(levels, lanes)
    rq_nodes = staged(nodes, fixed, CU_LDS)  # one block per CU
    s.update(rq_block=lanes, stack_lds=levels, rq_nodes=rq_nodes, rq_lds=fixed + 64 * rq_nodes)
    s["error"] = int(rq and s["rq_lds"] > CU_LDS)
    return s


BUILD_KNOBS = [{}, {"NART_RQ_LDS_LIMIT": str(100 * 1024)}, {"NART_LEAN_STACK": "3"}, {"NART_LEAN_STACK": ""},
               {"NART_LEAN_STACK": "20"}, {"NART_LEAN_ROUNDS": "0"}, {"NART_LEAN_ROUNDS": "0", "NART_LEAN_STACK": "3"}]
SCENES = [(FM_DIFFUSE, 0), (FT["lambert"], 0), (FM_GLASS, 0), (FM_DIFFUSE | FT["ring"], 0), (FT_ALL & ~FT["environment"], 0),
          (FM_ENVTEX, 1), (FT["lambert"] | FT["environment"], 1), (FM_GLASS | FT["environment"], 1), (FT_ALL, 1)]
# 25 / 26: the deepest stack the 512-lane layout holds (60 KiB + 4 KiB per level = 160 KiB at 25); 8 / 9
# and 10 / 11: the levels a 768-lane block holds beside 320 and beside 100 staged nodes
DEPTHS = (1, 3, 4, 5, 8, 9, 10, 11, 14, 24, 25, 26)
NODES = (0, 100, 319, 320, 759, 5000)


def _sizes(res_k):
    lanes = 256 * res_k
    out = {lanes // 2, lanes, lanes + 1}
    for t in (1.5, 3.0, 6.0, 12.0):  # rounds just below and at each threshold
        out |= {int(t * lanes) - 1, int(t * lanes)}
    return sorted(out | {14 * lanes + 7})


def _build_cases():
    # which build: every scene class, mode and size, on a BVH the ray-queue kernel holds and one it does not
    for res_k in (6, 512):
        for n, (features, env), depth in itertools.product(_sizes(res_k), SCENES, (14, 26)):
            for spec, counters, bounces, variant in itertools.product((OFF, ON, LEAN), (0, 1), (10, 11), (0, 3)):
                yield (features, env, spec, counters, bounces, variant, depth, 759, n, res_k), {}
            for spec, variant, kn in itertools.product((ON, LEAN), (0, 3), BUILD_KNOBS[1:]):
                yield (features, env, spec, 0, 10, variant, depth, 759, n, res_k), kn
    # which layout: every depth and node count, for each block size (512, 768 lean, 256 counting), a
    # launch below and one above every lean threshold
    for n, depth, nodes, kn in itertools.product((100 * 256, 14 * 512 * 256 + 7), DEPTHS, NODES, BUILD_KNOBS):
        for (features, env), spec, counters in itertools.product((SCENES[0], SCENES[2], SCENES[4], SCENES[5]), (ON, LEAN), (0, 1)):
            yield (features, env, spec, counters, 10, 0, depth, nodes, n, 512), kn


def _build_line(c, kn):
    rq_blocks = max(1, c[9] // 2)  # one ray-queue block per CU, two k_render blocks
    return "build %d %d %d %d %d %d %d %d %d %d" % c + " %d 1 " % rq_blocks + \
        " ".join(_knob(kn, k) for k in ("NART_RQ_LDS_LIMIT", "NART_LEAN_STACK", "NART_LEAN_ROUNDS"))


def test_plan_build_matches_the_policy_and_what_cannot_occur(checker):
    cases = list(_build_cases())
    seen, refused = set(), 0
    for (c, kn), line in zip(cases, checker([_build_line(c, kn) for c, kn in cases])):
        text, message = line.split(" # ") if not line.endswith(" # ") else (line[:-3], "")
        got = _fields(text)
        plan = {k[2:]: got.pop(k) for k in list(got) if k.startswith("p_")}
        want = restate_build(*c, kn=kn)
        assert got == want, (c, kn, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        assert message == (RANGE_ERROR if got["error"] else "")
        build = tuple(got[k] for k in ("ext", "count", "env", "fm", "wv", "pr"))
        assert build in BUILDS, (c, kn, build)  # render.hip has the instantiation
        features, env, spec, counters, bounces, variant, depth = c[:7]
        lean, names = got["wv"] == 3, {k for k, bit in SCHED.items() if plan["sched"] & bit}
        # every layout that is not refused can be launched
        if not got["error"]:
            assert 1 <= got["stack_lds"] <= depth and got["k_lds"] <= CU_LDS and (not got["rq"] or got["rq_lds"] <= CU_LDS)
        refused += got["error"]
        seen.add((build, got["rq"], plan["shape"]))
        # the lean choice tests the 512-lane layout; a 768-lane layout that does not fit is refused, never launched
        if got["error"]:
            assert lean and rq_fixed_lds(depth, 512) <= CU_LDS < rq_fixed_lds(got["stack_lds"], 768)
        # DESIGN.md's "cannot occur" cells
        if lean:
            assert got["rq"] and not got["pr"] and not got["ext"] and not got["count"] and got["fm"] != FT_ALL
        if got["count"]:
            assert got["fm"] == FT_ALL and got["rq_block"] == 256
        assert got["ext"] == int(bounces > 10)
        assert not plan["error"]
        if kn:
            continue
        k32 = plan["shape"] == PIXEL_QUEUE and plan["k"] == 32
        if lean:
            assert not names & {"priority", "spec_pairs", "half_waves"} and not k32
            assert not (plan["rq_prio"] or plan["pairs"] or plan["half"] or plan["quad"])
            assert "lean" in names
        if got["rq"] and not lean and spec == LEAN and got["fm"] in (FM_DIFFUSE, FM_ENVTEX):
            assert not k32 and "wave_groups" not in names, (c, plan)
    # the grid reaches every build on both kernels, each shape, and the refusal
    assert {s[0] for s in seen if s[1]} == BUILDS
    assert {s[0] for s in seen if not s[1]} == {b for b in BUILDS if b[4] == 2}  # k_render: never lean
    assert {s[2] for s in seen} >= {DIRECT, GROUPS, PIXEL_QUEUE} and refused


def test_plan_build_suite_scenes(checker):
    """The layouts the measurement notes state: C3 (14 levels, 759 nodes) keeps 8 levels and 352 nodes in
    the lean block's LDS; a 26-level BVH falls back to k_render."""
    c3, deep = checker([_build_line((FM_GLASS, 0, LEAN, 0, 5, 0, 14, 759, 1920 * 1080, 512), {}),
                        _build_line((FM_GLASS, 0, LEAN, 0, 5, 0, 26, 759, 1920 * 1080, 512), {})])
    c3, deep = _fields(c3.split(" # ")[0]), _fields(deep.split(" # ")[0])
    assert (c3["wv"], c3["rq_block"], c3["stack_lds"], c3["rq_nodes"], c3["rq_lds"]) == (3, 768, 8, 352, CU_LDS)
    assert (deep["rq"], deep["wv"], deep["fm"], deep["fm_used"]) == (0, 2, FM_GLASS, FT_ALL)


# ------------------------------------------------------------------ the volume launch, restated
def restate_volume(n, spp, resident, cells, counters, kn):
    blocks = -(-n // 256)
    v = dict(lds_nodes=cells if cells <= 4096 else 0, blocks=blocks, W=4 * resident, queue=0, queue_room=0,
             sparse=0, S=0, f=0.0, sched=0)
    # the four-wave build from 8 rounds, counted in whole blocks per resident block
    v["build"] = COUNTER if counters else (FOUR_WAVE if blocks / resident >= 8 else PLAIN)
    # the cost-probed queue: more blocks than resident, fewer than 12 rounds of slots, more samples than the probe's 4
    if blocks > resident and n / (256.0 * resident) < 12 and spp > 4:
        S = int(max(1.0, min(64.0, _num(kn, "NART_VOL_SPARSE", 16))))
        v.update(queue=1, queue_room=n + 63 * v["W"], sched=SCHED["vol_queue"], S=S, f=_num(kn, "NART_VOL_SPARSE_F", 4.0))
        # sparse waves: S pixels per wave must split a group of 64 evenly; shards below 2 rounds
        v["sparse"] = int(S < 64 and 64 % S == 0 and blocks / resident < _num(kn, "NART_VOL_SPARSE_ROUNDS", 2.0))
    return v


VOLUME_KNOBS = [{}] + [{"NART_VOL_SPARSE": s, "NART_VOL_SPARSE_ROUNDS": r, "NART_VOL_SPARSE_F": "1.1"}
                       for s, r in (("64", "2"), ("16", "8"), ("4", "8"))] + \
    [{"NART_VOL_SPARSE": s} for s in ("0", "1", "3", "8", "32", "48", "100", "")] + \
    [{"NART_VOL_SPARSE_ROUNDS": r} for r in ("1", "12.5")] + [{"NART_VOL_SPARSE_F": "2.5"}]


def _volume_cases():
    for resident in (6, 256):
        sizes = set()
        for t in (1, 2, 8, 12):  # whole blocks and slots disagree about the round when n is no multiple of 256
            m = t * 256 * resident
            sizes |= {m - 256, m - 255, m - 1, m, m + 1}
        for n, spp, cells, counters, kn in itertools.product(sorted(sizes), (4, 5, 1024), (0, 8, 4096, 4097), (0, 1),
                                                             VOLUME_KNOBS):
            yield (n, spp, resident, cells, counters), kn


def test_plan_volume_matches_the_policy(checker):
    cases = list(_volume_cases())
    lines = ["volume %d %d %d %d %d " % c + " ".join(_knob(kn, "NART_VOL_SPARSE" + s) for s in ("", "_F", "_ROUNDS"))
             for c, kn in cases]
    seen = set()
    for (c, kn), line in zip(cases, checker(lines)):
        got, want = _fields(line), restate_volume(*c, kn=kn)
        assert got == want, (c, kn, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        seen.add((got["build"], got["queue"], got["sparse"]))
    # (four waves and sparse waves together only with NART_VOL_SPARSE_ROUNDS > 8)
    assert seen == {(b, q, s) for b in (COUNTER, FOUR_WAVE, PLAIN) for q, s in ((0, 0), (1, 0), (1, 1))}
    # n = 8 rounds of blocks but fewer of slots, and the reverse at 12
    res = 6
    a, b = checker(["volume %d 8 %d 8 0 - - -" % (8 * 256 * res - 255, res), "volume %d 8 %d 8 0 - - -" % (12 * 256 * res - 1, res)])
    assert _fields(a)["build"] == FOUR_WAVE and _fields(b)["queue"] == 1


def restate_hot(keys, f, S, W, n):
    """keys: 0xFFFFFFFE - cost of each 64-slot group, ascending (costliest first); a partial last group
    has the key 0xFFFFFFFF and never counts."""
    costs = [0xFFFFFFFE - k for k in keys if k != 0xFFFFFFFF]
    dense = dict(H=0, qlen=0, grid=-(-n // 256))
    if not costs:
        return dense
    median = costs[len(costs) // 2]
    hot = sum(1 for c in costs if c >= f * median)  # a prefix: the costs descend
    # a hot group takes 64 / S waves, 64 / S - 1 of them beyond its own: the queue has 63 W entries beyond n
    hot = min(hot, 63 * W // (64 // S * 64))
    if not hot:
        return dense
    qlen = hot * (64 // S) * 64 + n - 64 * hot
    return dict(H=hot, qlen=qlen, grid=-(-qlen // 256))


def test_sparse_hot_groups(checker):
    def keys_of(costs, n):
        ks = sorted(0xFFFFFFFE - c for c in costs)
        return ks + ([0xFFFFFFFF] if n % 64 else [])

    cases = []
    for S, W in itertools.product((1, 2, 4, 16, 32), (1, 4, 24, 1024)):
        for f in (1.1, 4.0):
            cases += [
                (f, S, W, 64 * 40, keys_of([1000] * 3 + [900, 500] + [100] * 35, 64 * 40)),   # a few hot groups
                (f, S, W, 64 * 40 + 17, keys_of([5000] * 30 + [100] * 10, 64 * 40 + 17)),     # many: capped; partial last group
                (f, S, W, 17, keys_of([], 17)),                                                # only a partial group: no costs
                (f, S, W, 64 * 3, keys_of([0, 0, 0], 64 * 3)),                                 # every cost 0: all >= f x median
                (f, S, W, 64 * 5 + 1, keys_of([7, 7, 7, 7, 7], 64 * 5 + 1)),
                (f, S, W, 64 * 2, keys_of([0xFFFFFFFE, 1], 64 * 2)),                           # a saturated cost
            ]
    lines = ["hot %r %d %d %d " % c[:4] + " ".join(map(str, c[4])) for c in cases]
    capped = uncapped = 0
    for (f, S, W, n, keys), line in zip(cases, checker(lines)):
        got, want = _fields(line), restate_hot(keys, f, S, W, n)
        assert got == want, ((f, S, W, n), got, want)
        if got["H"]:
            assert got["qlen"] <= n + 63 * W  # ensure_queue's size (plan_volume's queue_room)
            wanted = sum(1 for k in keys if k != 0xFFFFFFFF and 0xFFFFFFFE - k >= f * (0xFFFFFFFE - keys[len([x for x in keys if x != 0xFFFFFFFF]) // 2]))
            capped += got["H"] < wanted
            uncapped += got["H"] == wanted
    assert capped and uncapped
