"""Cost of the cost image next to plain renders: render_ms (wall), kernel_ms (the path kernels, k_primary
included where it runs) and primary_ms of render_cost against a plain render and against the counter pass
(set_counters(True): what a user has without the feature, and totals only) on one context, for the
materials scene and veach at 1920x1080 / 16 spp; the median of --reps after a warm-up of each.  reduce_ms is
k_cost_reduce's share, so kernel_ratio says what the path kernel itself costs (no k_primary, one record
store per sample, the LDS adds) and reduce_ms what the grid costs.  --parent measures the plain render and
the counter pass alone: run it on the parent's build (NART_HIP_LIB) in the same session, alternating, to
see that a plain render did not get slower.  Prints one JSON line; a development aid, not the bench
contract."""
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
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    med = statistics.median
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree"), "frame": "%dx%d, %d spp" % (a.width, a.height, a.spp),
           "reps": a.reps}

    def measure(call):
        def once():
            st = nart_amd.RenderStats()
            call(st)
            return st.render_ms, st.kernel_ms, st.primary_ms
        once()  # warm-up
        t = [once() for _ in range(a.reps)]
        return {"ms": med(x[0] for x in t), "kernel_ms": med(x[1] for x in t), "primary_ms": med(x[2] for x in t),
                "ms_all": [round(x[0], 2) for x in t]}

    for name, path in (("materials", scenes.materials()), ("veach", scenes.reference_scene("veach"))):
        scene = nart_amd.Scene(path)
        r = nart_amd.HipRenderer(scene)
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = a.width, a.height, a.spp
        out = res[name] = {"bounces": p.bounces}
        out["render"] = measure(lambda st: r.render(p, stats=st))
        r.set_counters(True)
        out["counter_pass"] = measure(lambda st: r.render(p, stats=st))
        r.set_counters(False)
        if not a.parent:
            c = out["cost"] = measure(lambda st: r.render_cost(p, stats=st))
            c["reduce_ms"] = r.cost_timings()["reduce_ms"]
            c["ratio"] = c["ms"] / out["render"]["ms"]
            c["kernel_ratio"] = c["kernel_ms"] / out["render"]["kernel_ms"]
            c["ratio_to_counter_pass"] = c["ms"] / out["counter_pass"]["ms"]
        r.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
