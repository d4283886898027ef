"""Cost of depth cuts next to plain renders: render_ms (wall) and kernel_ms (the path kernels) of
render_depth_cuts against render on one context, for the materials scene and veach with K = 1 (direct
light: cuts [1]) and K = 4 (cuts [1, 2, 3, 5]) at 1920x1080 / 16 spp; the median of --reps after a warm-up
of each.  What a user does without the feature is K + 1 plain renders at lower bounce limits -- which do
not give the same split, since a pixel's later samples then trace other paths -- so the figures to read
are ratio = t(depth cuts) / t(render) against K + 1, and kernel_ratio and splat_ms for where the time
goes.  --plain-only measures the plain render alone: run it on the parent's build (NART_HIP_LIB) in the
same session to see that a plain render did not get slower.  Prints one JSON line; a development aid, not
the bench contract."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nart_amd  # noqa: E402
from nart_amd import scenes  # noqa: E402

CUTS = {1: [1], 4: [1, 2, 3, 5]}


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

    for name, path in (("materials", scenes.materials()), ("veach", scenes.reference_scene("veach"))):
        scene = nart_amd.Scene(path)
        r = nart_amd.HipRenderer(scene)
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = a.width, a.height, a.spp
        plain = lambda st: r.render(p, stats=st)  # noqa: E731
        timed(plain)  # warm-up
        t = [timed(plain) for _ in range(a.reps)]
        res[name] = {"bounces": p.bounces, "render_ms": med(x[0] for x in t), "render_kernel_ms": med(x[1] for x in t),
                     "render_ms_all": [x[0] for x in t]}
        for K, cuts in sorted(CUTS.items()):
            if a.plain_only:
                break
            cut = lambda st: r.render_depth_cuts(p, cuts, stats=st)  # noqa: E731
            timed(cut)  # warm-up
            t = [timed(cut) for _ in range(a.reps)]
            k = {"cuts": cuts, "depth_cuts_ms": med(x[0] for x in t), "depth_cuts_kernel_ms": med(x[1] for x in t),
                 "depth_cuts_ms_all": [x[0] for x in t], "splat_ms": r.depth_cut_timings()["splat_ms"]}
            k["ratio"] = k["depth_cuts_ms"] / res[name]["render_ms"]
            k["kernel_ratio"] = k["depth_cuts_kernel_ms"] / res[name]["render_kernel_ms"]
            res[name]["K%d" % K] = k
        r.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
