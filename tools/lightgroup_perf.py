"""Cost of light groups next to plain renders: render_ms (wall) of render_light_groups against render on
one context, for the materials scene with 2 groups and veach with 4 (one per light) at 1920x1080 / 16
spp; the median of --reps after a warm-up of each.  The yardstick is what a user does without the
feature: G plain renders of the frame, one per group with the other lights dark, so the figure to read
is ratio = t(light groups) / t(render) against G.  --plain-only measures the plain render alone: run it
on the parent's build (NART_HIP_LIB) in the same session to see that a plain render did not get slower.
Prints one JSON line; a development aid, not the bench contract."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nart_amd  # noqa: E402
from nart_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    med = statistics.median
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree"), "frame": "%dx%d, %d spp" % (a.width, a.height, a.spp),
           "reps": a.reps}

    def timed(call):
        st = nart_amd.RenderStats()
        call(st)
        return st.render_ms, st.kernel_ms

    for name, path, groups in (("materials", scenes.materials(), [0, 1]),
                               ("veach", scenes.reference_scene("veach"), [0, 1, 2, 3])):
        scene = nart_amd.Scene(path)
        r = nart_amd.HipRenderer(scene)
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = a.width, a.height, a.spp
        plain = lambda st: r.render(p, stats=st)  # noqa: E731
        grouped = lambda st: r.render_light_groups(p, groups, stats=st)  # noqa: E731
        timed(plain)  # warm-up
        t = [timed(plain) for _ in range(a.reps)]
        res[name] = {"groups": len(groups), "render_ms": med(x[0] for x in t), "render_kernel_ms": med(x[1] for x in t),
                     "render_ms_all": [x[0] for x in t]}
        if not a.plain_only:
            timed(grouped)  # warm-up
            t = [timed(grouped) for _ in range(a.reps)]
            res[name].update({"light_groups_ms": med(x[0] for x in t), "light_groups_kernel_ms": med(x[1] for x in t),
                              "light_groups_ms_all": [x[0] for x in t], "splat_ms": r.light_group_timings()["splat_ms"]})
            res[name]["ratio"] = res[name]["light_groups_ms"] / res[name]["render_ms"]
            res[name]["kernel_ratio"] = res[name]["light_groups_kernel_ms"] / res[name]["render_kernel_ms"]
        r.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
