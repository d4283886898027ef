"""Every build of the path kernels through every schedule shape, and the counter pass.

The parity bar is only as wide as the code objects and scheduling paths the suite drives.
render.hip dispatch_megakernel / launch_render compile the ray-queue kernel k_render_rq as the generic
two-wave build (FT_ALL) x {plain, EXT (overflow dielectric lists), COUNT (counter pass, 256-lane
blocks)} x {area lights, ENV}, and as FM_DIFFUSE / FM_GLASS / FM_ENVTEX, each two-wave (512 lanes) and
lean (768 lanes, no priority lanes); host/path_schedule.h plan_path sends a launch down Direct,
PixelQueue (priority lanes, speculative pairs / quads, half waves), Groups (orders 0-2) or
WholeGroupsByCost.  Each test below is one cell of that product (DESIGN.md "Build x schedule
coverage" lists them):

  * the reference is the oracle's whole frame, compared as uint32 bits, tolerance 0;
  * every cell asserts the build it ran (HipRenderer.scene_features()[1]) and the path it took
    (RenderStats.schedule_names()), so it cannot silently test a neighbouring cell.

Frame sizes are the smallest of a handful tried on an MI355X (256 CUs) whose schedule_names() show
the wanted path.  "Rounds" are rounds of k_render's resident lanes (plan_path's R), one round being
about 131-132 thousand traced pixels there (a 416x300 frame, 127,680 slots, is still Direct;
432x300, 132,544, is queued):

    432x300    132,544 slots  1.0 rounds  pixel queue, k = 12 half waves (two-wave builds)
    496x312    158,000        1.2         the same, the NART_QUEUE_K layouts
    520x380    201,216        1.5         lean build's pixel queue (its grid holds 196,608 lanes)
    768x508    395,264        3.0         k = 32 queue (760x512, 394,224, is still below 3 rounds)
    1056x750   799,240        6.1         wave groups (1040x750, 787,176, is still the k = 32 queue)
    256x240     63,440        0.5         counter pass, Direct (its 256-lane grid holds 65,536 lanes)
    260x250     67,056        0.5         counter pass, pixel queue with half waves

A speculative pair's second lane joins only once its pixel has a committed sample to predict from, so
at 1 or 2 spp a pair never holds a speculative job (measured: at 2 spp the counter pass's path counts
did not change with NART_RQ_PAIRS, at 8 spp they did).  Cells whose point is the pairs therefore run
3-8 spp, as their docstrings say; the others 1 spp.  Oracle frames are rendered once per module and
shared (the `frames` fixture); the wall times in the docstrings are from one MI355X run and include
the oracle frame where the test is the first to ask for it.
"""
import numpy as np
import pytest

import nart_amd
import oracle
from nart_amd import scenes

pytestmark = pytest.mark.gpu

FT = nart_amd.api.FEATURES
FT_ALL = nart_amd.api.FT_ALL
FM_DIFFUSE = FT["lambert"] | FT["disk"]
FM_GLASS = FT["lambert"] | FT["glass"] | FT["disk"]

# the schedule bits that name a path-kernel build or scheduling path (the others: k_primary, splats)
PATH_BITS = {"lean", "specialized", "probe_queue", "priority", "spec_pairs", "half_waves", "wave_groups"}
HALF = {"probe_queue", "priority", "spec_pairs", "half_waves"}
PAIRS = {"probe_queue", "priority", "spec_pairs"}
KNOBS = ("NART_RQ_PRIO", "NART_RQ_PAIRS", "NART_RQ_HALF", "NART_RQ_QUAD", "NART_RQ_SETPRIO", "NART_RQ_ORDER",
         "NART_RQ_TOPF", "NART_PROBE_SUB", "NART_QUEUE_K", "NART_LEAN_ROUNDS", "NART_LEAN_STACK", "NART_PRIMARY_PACKET")
PATH_COUNTERS = ("rays_extend", "rays_shadow", "bounces")
TRAVERSAL_COUNTERS = ("node_visits", "tri_tests", "octree_checks", "octree_replays")


def _params(scene, w, h, spp, **kw):
    p = nart_amd.load_sessions(scene.path)[0]
    p.image_width, p.image_height, p.spp = w, h, spp
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _slots(p):
    g = nart_amd.session_geometry(p)
    return g.total_width * g.total_height  # traced pixels: the extra rows and columns count


def _report(a, b):
    ne = a.view(np.uint32) != b.view(np.uint32)
    return "%d of %d floats differ, max abs diff %g" % (int(ne.sum()), ne.size, float(np.nanmax(np.abs(a - b))))


def _assert_bits(a, b):
    assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), _report(a, b)


@pytest.fixture(autouse=True)
def clean_knobs(monkeypatch):
    """Every cell starts from the default schedule: no knob of the caller's environment leaks in."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def frames():
    """oracle_frame(scene, p) -> (image, path counts, longest dielectric list): each oracle frame of
    the module rendered once, read-only, shared by the cells that use it."""
    cache = {}

    def oracle_frame(scene, p):
        key = (scene.path, p.image_width, p.image_height, p.spp, p.bounces)
        if key not in cache:
            counts = {}
            oracle.max_list_length(reset=True)
            img = oracle.Oracle(scene).render(p, counts=counts)
            img.setflags(write=False)
            cache[key] = (img, counts, oracle.max_list_length())
        return cache[key]

    return oracle_frame


@pytest.fixture(scope="module")
def nested10_scene(built, tmp_path_factory):
    return nart_amd.Scene(scenes.nested_glass(str(tmp_path_factory.mktemp("nest10")), spp=1, bounces=10))


@pytest.fixture(scope="module")
def nested16_scene(built, tmp_path_factory):
    return nart_amd.Scene(scenes.nested_glass(str(tmp_path_factory.mktemp("nest16")), spp=1, bounces=16))


def _render(scene, p, variant=0, specialize=None, counters=False):
    """(image, stats, mask of the build that ran, path names) of one render on a fresh context."""
    r = nart_amd.HipRenderer(scene, variant=variant)
    if specialize is not None:
        r.set_specialize(specialize)
    if counters:
        r.set_counters(True)
    st = nart_amd.RenderStats()
    img = r.render(p, st)
    build = r.scene_features()[1]
    r.close()
    return img, st, build, set(st.schedule_names()) & PATH_BITS


# ---------------------------------------------------------------- A. generic build, every schedule shape

@pytest.mark.parametrize("pairs,path", [(None, HALF), ("4", PAIRS), ("0", HALF - {"spec_pairs"})],
                         ids=["default", "quads", "single-lanes"])
def test_generic_pixel_queue_materials(gpu, materials_scene, frames, monkeypatch, pairs, path):
    """Generic two-wave build (FT_ALL, 512 lanes) through the default pixel queue below 3 rounds:
    materials at 432x300 (132,544 slots, 1.0 rounds: the smallest queued frame), 4 spp so that the
    pairs / quads hold speculative jobs.  Priority lanes on half waves with pairs; NART_RQ_PAIRS=4
    (four lanes per costly pixel, no half waves: 2 shares x 4 x 12 > 64); NART_RQ_PAIRS=0 (one lane each).
    Wall time: 0.3 s the first (oracle frame), 0.01 s the others."""
    if pairs is not None:
        monkeypatch.setenv("NART_RQ_PAIRS", pairs)
    p = _params(materials_scene, 432, 300, 4)
    g, st, build, names = _render(materials_scene, p)
    assert build == FT_ALL and names == path, (hex(build), names)
    _assert_bits(g, frames(materials_scene, p)[0])


def test_generic_k32_queue_materials(gpu, materials_scene, frames):
    """Generic build through the k = 32 queue between 3 and 6 rounds (no priority lanes): materials at
    768x508 (395,264 slots, 3.0 rounds: the smallest frame past the threshold), 1 spp.  Wall time 0.12 s."""
    p = _params(materials_scene, 768, 508, 1)
    g, st, build, names = _render(materials_scene, p)
    assert build == FT_ALL and names == {"probe_queue"}, (hex(build), names)
    _assert_bits(g, frames(materials_scene, p)[0])


@pytest.mark.parametrize("order", ["0", "1", "2"], ids=["slot-order", "costliest-first", "top-class-first"])
def test_generic_wave_groups_materials(gpu, materials_scene, frames, monkeypatch, order):
    """Generic build through the wave-group refill from 6 rounds, groups in slot order, costliest
    first, or the costliest NART_RQ_TOPF % first: materials at 1056x750 (799,240 slots, 6.1 rounds:
    the smallest frame that takes groups), 1 spp.  Wall time 0.25 s the first (oracle frame), up to 0.04 s the others."""
    monkeypatch.setenv("NART_RQ_ORDER", order)
    monkeypatch.setenv("NART_RQ_TOPF", "15")
    p = _params(materials_scene, 1056, 750, 1)
    g, st, build, names = _render(materials_scene, p)
    assert build == FT_ALL and names == {"wave_groups"}, (hex(build), names)
    _assert_bits(g, frames(materials_scene, p)[0])


def test_generic_speculative_pairs_glass(gpu, glass_scene, frames):
    """glassSphere with set_specialize(False): test_queue_speculative_pairs's `speculative-pairs`
    configuration (default knobs) on the generic build, at 24 spp so that speculation is both kept
    and dropped; 432x300 (132,544 slots, 1.0 rounds).  The 24-spp oracle frame of this glass scene
    is the slow part (3.2 M samples); the spp is the cell's point, so it stays.  Wall time 4.1 s."""
    p = _params(glass_scene, 432, 300, 24)
    g, st, build, names = _render(glass_scene, p, specialize=False)
    assert build == FT_ALL and names == HALF, (hex(build), names)
    _assert_bits(g, frames(glass_scene, p)[0])


def test_generic_wave_groups_glass(gpu, glass_scene, frames):
    """glassSphere with set_specialize(False) through wave groups in the default order (costliest
    group first): 1056x750 (799,240 slots, 6.1 rounds), 1 spp.  Wall time 1.1 s (oracle frame)."""
    p = _params(glass_scene, 1056, 750, 1)
    g, st, build, names = _render(glass_scene, p, specialize=False)
    assert build == FT_ALL and names == {"wave_groups"}, (hex(build), names)
    _assert_bits(g, frames(glass_scene, p)[0])


# ---------------------------------------------------------------- B. lean build off its beaten track

@pytest.mark.parametrize("lds_levels", ["2", None], ids=["2-lds-levels", "default-stack"])
def test_lean_nested_glass(gpu, nested10_scene, frames, monkeypatch, lds_levels):
    """Lean FM_GLASS build (NART_LEAN_ROUNDS=0) on nested_glass(bounces=10): the compact dielectric
    list with real nesting (kernels.h IList's penId / mesh_eta path) and, with 2 LDS stack levels,
    nearly every traversal push in the per-thread global columns.  520x380 (201,216 slots: more than
    the lean grid's 196,608 lanes, 1.5 rounds), 1 spp: the lean pixel queue, whose lanes refill.
    Against the oracle and against the generic build.  Wall time 0.25 s the first (oracle frame), 0.01 s the second."""
    monkeypatch.setenv("NART_LEAN_ROUNDS", "0")
    if lds_levels:
        monkeypatch.setenv("NART_LEAN_STACK", lds_levels)
    p = _params(nested10_scene, 520, 380, 1)
    g, st, build, names = _render(nested10_scene, p)
    assert build == FM_GLASS and names == {"lean", "specialized", "probe_queue"}, (hex(build), names)
    ref, _, longest = frames(nested10_scene, p)
    assert longest >= 8, longest  # real nesting (14 shells, 10 bounces): the register list all but full
    _assert_bits(g, ref)
    gen, _, gbuild, gnames = _render(nested10_scene, p, specialize=False)
    assert gbuild == FT_ALL and "lean" not in gnames, (hex(gbuild), gnames)
    _assert_bits(g, gen)


RAGGED = [(8, 8), (20, 16), (37, 29), (61, 45), (90, 70)]


@pytest.mark.parametrize("which,mask", [("glass", FM_GLASS), ("cornell", FM_DIFFUSE)], ids=["glass", "cornell"])
def test_lean_ragged_direct_launches(gpu, glass_scene, cornell_scene, frames, monkeypatch, which, mask):
    """The lean build never runs below its round thresholds by default, so never a partly filled
    768-lane block: forced (NART_LEAN_ROUNDS=0) on tiny Direct frames of 144 and 480 slots (less than
    one block) and 1,353 / 3,185 / 6,956 slots (1, 4 and 9 whole blocks plus 585, 113 and 44 lanes),
    2 spp.  Wall time for the five frames and their oracle frames: 0.18 s glassSphere, 0.04 s Cornell."""
    monkeypatch.setenv("NART_LEAN_ROUNDS", "0")
    sc = glass_scene if which == "glass" else cornell_scene
    tails = []
    for w, h in RAGGED:
        p = _params(sc, w, h, 2)
        n = _slots(p)
        tails.append((n // 768, n % 768))
        g, st, build, names = _render(sc, p)
        assert build == mask and names == {"lean", "specialized"}, (w, h, hex(build), names)
        _assert_bits(g, frames(sc, p)[0])
    assert all(t for _, t in tails) and sum(b == 0 for b, _ in tails) >= 1 and sum(b > 0 for b, _ in tails) >= 2, tails


@pytest.mark.parametrize("order", ["0", "2"], ids=["slot-order", "top-class-first"])
def test_lean_wave_group_orders(gpu, glass_scene, frames, monkeypatch, order):
    """The lean build's wave groups in slot order and with the costliest class first (the suite
    otherwise runs only its default, order 1): glassSphere, lean forced, 1056x750 (6.1 rounds; the
    lean build takes groups from 3), 1 spp, the oracle frame of test_generic_wave_groups_glass.
    Wall time 0.01 s."""
    monkeypatch.setenv("NART_LEAN_ROUNDS", "0")
    monkeypatch.setenv("NART_RQ_ORDER", order)
    p = _params(glass_scene, 1056, 750, 1)
    g, st, build, names = _render(glass_scene, p)
    assert build == FM_GLASS and names == {"lean", "specialized", "wave_groups"}, (hex(build), names)
    _assert_bits(g, frames(glass_scene, p)[0])


# ---------------------------------------------------------------- C. overflow lists on a persistent grid

@pytest.mark.parametrize("variant", [0, 3], ids=["rayqueue", "megakernel"])
@pytest.mark.parametrize("w,h,spp,path", [(432, 300, 3, HALF), (1056, 750, 1, {"wave_groups"})],
                         ids=["pixel-queue", "wave-groups"])
def test_overflow_lists_persistent_grid(gpu, nested16_scene, frames, variant, w, h, spp, path):
    """EXT builds (bounces 16 > ILIST_REG: list entries beyond 10 in per-thread global columns
    indexed by the global thread id) on a persistent grid: nested_glass(bounces=16) through the
    default pixel queue (432x300, 1.0 rounds, 3 spp: priority lanes, speculative pairs, refill)
    and through wave groups (1056x750, 6.1 rounds, 1 spp).  The one-lane-per-pixel kernel (variant 3)
    runs both frames through its own refilling pixel queue.  Wall time 0.5 s / 1.1 s for the first of
    each frame (oracle), 0.01 s the second."""
    p = _params(nested16_scene, w, h, spp)
    g, st, build, names = _render(nested16_scene, p, variant=variant)
    assert build == FT_ALL and names == (path if variant == 0 else {"probe_queue"}), (hex(build), names)
    ref, _, longest = frames(nested16_scene, p)
    assert longest > 10, longest  # the overflow entries were really used
    _assert_bits(g, ref)


# ---------------------------------------------------------------- D. NART_QUEUE_K on the device

QK_FRAME = (496, 312, 8)  # 158,000 slots, 1.2 rounds; 8 spp: see test_counts_schedule_invariance


@pytest.mark.parametrize("env,path", [
    ({"NART_QUEUE_K": "1"}, HALF),
    ({"NART_QUEUE_K": "64"}, set()),
    ({"NART_QUEUE_K": "31", "NART_RQ_PRIO": "2", "NART_RQ_QUAD": "1"}, PAIRS),
    ({"NART_QUEUE_K": "20", "NART_RQ_PAIRS": "4"}, {"probe_queue", "priority"})],
    ids=["k1", "k64-whole-groups", "k31-quad", "k20-pairs-dropped"])
def test_queue_k_on_device(gpu, glass_scene, frames, monkeypatch, env, path):
    """Queue layouts plan_path is only planned with elsewhere, launched: one costly pixel per wave
    (k = 1); k = 64, WholeGroupsByCost (one lane per pixel, groups launched costliest first: no
    probe_queue bit); k = 31 with forced priority and a four-lane group for each wave's costliest
    pixel (2 x 31 + 2 = 64 lanes); k = 20 with NART_RQ_PAIRS=4, whose groups are dropped because
    4 x 20 > 64.  glassSphere (FM_GLASS build), 496x312 (158,000 slots, 1.2 rounds), 8 spp so the
    pair and quad lanes speculate.  Wall time 1.6 s the first (oracle frame), 0.01 s the others."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = _params(glass_scene, *QK_FRAME)
    g, st, build, names = _render(glass_scene, p)
    assert build == FM_GLASS and names == path | {"specialized"}, (hex(build), names)
    _assert_bits(g, frames(glass_scene, p)[0])


# ---------------------------------------------------------------- E. the counter pass

def _counts(st):
    return {k: getattr(st, k) for k in PATH_COUNTERS + TRAVERSAL_COUNTERS + ("traced_samples",)}


def _assert_counts_match_oracle(st, oc):
    """rays_extend, bounces ("shaded" hits: every extension query that found a surface, nart_hip.h)
    and traced_samples equal the oracle's; rays_shadow is bounded by its visibility queries (the
    device skips occlusion queries whose term is exactly zero)."""
    got = (st.rays_extend, st.bounces, st.traced_samples)
    assert got == (oc["extension_queries"], oc["shaded_hits"], oc["traced_samples"]), (got, oc)
    assert 0 < st.rays_shadow <= oc["visibility_queries"], (st.rays_shadow, oc)


COUNTER_SHAPES = [(256, 240, 1, set()), (260, 250, 4, HALF), (1056, 750, 1, {"wave_groups"})]


@pytest.mark.parametrize("w,h,spp,path", COUNTER_SHAPES, ids=["direct", "half-waves", "wave-groups"])
@pytest.mark.parametrize("which", ["glass", "materials", "env"])
def test_counter_pass_image_and_counts(gpu, glass_scene, materials_scene, env_scene, frames, which, w, h, spp, path):
    """The counter pass's own code objects (COUNT: always generic, 256-lane ray-queue blocks, one per
    CU, so its grid holds 65,536 lanes) render the oracle's image and report the oracle's path counts:
    Direct (256x240, 63,440 slots), the pixel queue with half waves (260x250, 67,056 slots, 4 spp so
    the pairs speculate; in 256-lane blocks every wave is one of the first four), wave groups
    (1056x750, 6.1 rounds).  Wall time 0.01-0.14 s; 0.43 s for glassSphere's half waves (oracle frame)."""
    sc = {"glass": glass_scene, "materials": materials_scene, "env": env_scene}[which]
    p = _params(sc, w, h, spp)
    g, st, build, names = _render(sc, p, counters=True)
    assert build == FT_ALL and names == path, (hex(build), names)
    ref, oc, _ = frames(sc, p)
    _assert_bits(g, ref)
    _assert_counts_match_oracle(st, oc)


@pytest.mark.parametrize("which", ["glass", "materials", "env"])
def test_counter_pass_variants_agree(gpu, glass_scene, materials_scene, env_scene, frames, which):
    """k_render (variant 3) and k_render_rq are two independently written kernels: the same
    rays_shadow exactly (the oracle only bounds it), and k_render's path counts equal the oracle's
    too.  The 260x250x4 frame of test_counter_pass_image_and_counts: the pixel queue with speculative
    pairs for k_render_rq, one lane per pixel (Direct: k_render's grid holds a whole round) for
    k_render.  Wall time 0.01 s."""
    sc = {"glass": glass_scene, "materials": materials_scene, "env": env_scene}[which]
    p = _params(sc, 260, 250, 4)
    g0, st0, build0, names0 = _render(sc, p, variant=0, counters=True)
    g3, st3, build3, names3 = _render(sc, p, variant=3, counters=True)
    assert build0 == FT_ALL and build3 == FT_ALL and names0 == HALF and names3 == set(), (names0, names3)
    ref, oc, _ = frames(sc, p)
    _assert_bits(g3, ref)
    _assert_counts_match_oracle(st3, oc)
    assert {k: getattr(st0, k) for k in PATH_COUNTERS} == {k: getattr(st3, k) for k in PATH_COUNTERS}


INVARIANCE = [({"NART_RQ_PAIRS": "0"}, HALF - {"spec_pairs"}, False), ({"NART_RQ_PAIRS": "2"}, HALF, True),
              ({"NART_RQ_PAIRS": "4"}, HALF, True), ({"NART_RQ_PRIO": "0"}, {"probe_queue"}, False),
              ({"NART_RQ_PRIO": "1"}, HALF, True), ({"NART_QUEUE_K": "64"}, set(), False)]


def test_counts_schedule_invariance(gpu, glass_scene, frames, monkeypatch):
    """rays_extend, rays_shadow and bounces are properties of the scene and the session, not of the
    schedule a launch happened to take: identical with NART_RQ_PAIRS 0 / 2 / 4, NART_RQ_PRIO 0 / 1
    and NART_QUEUE_K=64, and equal to the oracle's (in the counter pass's 256-lane blocks one share of
    8 costly pixels x 4 lanes fits a wave, so the quads too run on half waves).  node_visits, tri_tests, octree_checks and
    octree_replays are added by whichever lane traces a ray (nart_hip.h): identical across the
    settings without speculation, and no smaller with it.  glassSphere, 496x312 (1.2 rounds), 8 spp:
    at 2 spp no pair holds a speculative job; at 8 spp, before k_render_rq held a speculative
    sample's counts back until the sample was accepted, pairs reported rays_extend 2,854,542 and
    quads 2,915,336 where the settings without speculation (and the oracle) count 2,823,349.
    Wall time 0.05 s (the oracle frame is test_queue_k_on_device's)."""
    p = _params(glass_scene, *QK_FRAME)
    _, oc, _ = frames(glass_scene, p)
    runs = []
    for env, path, speculates in INVARIANCE:
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            _, st, build, names = _render(glass_scene, p, counters=True)
        assert build == FT_ALL and names == path, (env, hex(build), names)
        _assert_counts_match_oracle(st, oc)
        runs.append((env, speculates, _counts(st)))
    first = runs[0][2]
    for env, speculates, c in runs[1:]:
        assert {k: c[k] for k in PATH_COUNTERS} == {k: first[k] for k in PATH_COUNTERS}, (env, c, first)
        if not speculates:
            assert c == first, (env, c, first)
        else:
            assert all(c[k] >= first[k] for k in TRAVERSAL_COUNTERS), (env, c, first)


def test_counts_no_carry_over(gpu, glass_scene, frames):
    """Two renders in a row on one context report the same counts (the device counters are zeroed
    per render), and a counter-free render in between reports none.  The 260x250x4 frame.
    Wall time 0.01 s."""
    p = _params(glass_scene, 260, 250, 4)
    r = nart_amd.HipRenderer(glass_scene)
    r.set_counters(True)
    seen = []
    for counters in (True, True, False, True):
        r.set_counters(counters)
        st = nart_amd.RenderStats()
        g = r.render(p, st)
        build, names = r.scene_features()[1], set(st.schedule_names()) & PATH_BITS
        if counters:
            assert build == FT_ALL and names == HALF, (hex(build), names)
            seen.append(_counts(st))
        else:
            assert build == FM_GLASS and "specialized" in names, (hex(build), names)
            assert not any(getattr(st, k) for k in PATH_COUNTERS + TRAVERSAL_COUNTERS), _counts(st)
        _assert_bits(g, frames(glass_scene, p)[0])
    r.close()
    assert seen[0] == seen[1] == seen[2], seen
    _assert_counts_match_oracle(st, frames(glass_scene, p)[1])
