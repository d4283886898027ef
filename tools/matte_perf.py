"""Cost of the first-hit ID mattes next to a first-hit AOV: matte_ms (the plane passes: k_matte_ids +
splat per plane) and rank_ms of a matte-only nart_hip_render_mattes, and aov_ms of an albedo-only
render_aovs of the same frame (one k_aov + splat), for glassSphere and the materials scene (one and
two planes) at 1920x1080 / 4 spp.  --aov-only measures the AOV alone: run it on the parent's build
(NART_HIP_LIB) in the same session for the yardstick.  Prints one JSON line; a development aid, not the
bench contract."""
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
    ap.add_argument("--aov-only", action="store_true")
    a = ap.parse_args()
    med = statistics.median
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree"), "frame": "1920x1080, 4 spp", "reps": a.reps}
    for name, path in (("glassSphere", scenes.glass_sphere()), ("materials", scenes.materials())):
        scene = nart_amd.Scene(path)
        r = nart_amd.HipRenderer(scene)
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, 4
        r.render_aovs(p, normal=False, beauty=False)  # warm-up
        aov = [r.render_aovs(p, normal=False, beauty=False)["aov_ms"] for _ in range(a.reps)]
        res[name] = {"albedo_aov_ms": med(aov), "albedo_aov_ms_all": aov}
        if not a.aov_only:
            r.render_mattes(p)  # warm-up
            matte, rank, n = [], [], 0
            for _ in range(a.reps):
                out = r.render_mattes(p)
                matte.append(out["matte_ms"])
                rank.append(out["rank_ms"])
                n = out["n_ids"]
            planes = (n + 3) // 4
            res[name].update({"n_ids": n, "planes": planes, "ranks": 6, "matte_ms": med(matte), "rank_ms": med(rank),
                              "matte_ms_all": matte, "rank_ms_all": rank,
                              "matte_ms_per_plane_over_aov_ms": med(matte) / planes / med(aov)})
        r.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
