"""Cost of the firefly cascade next to what it sits beside: cascade_ms (the split and the K layer
splats), reweight_ms and splat_ms (the beauty's splat + combine) of the same frames, at 1920x1080 /
4 spp and on the C3 frame (glassSphere 1920x1080, 256 spp), with the default parameters (K = 6).
--plain-only measures the plain render's splat_ms alone: run it on the parent's build (NART_HIP_LIB)
in the same session for the yardstick.  Prints one JSON line; a development aid, not the bench
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--c3-reps", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    path = scenes.glass_sphere()
    scene = nart_amd.Scene(path)
    r = nart_amd.HipRenderer(scene)
    med = statistics.median
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree")}
    for name, spp, reps in (("1080p_4spp", 4, a.reps), ("c3", 256, a.c3_reps)):
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, spp
        r.render(p)  # warm-up
        plain_splat, kernel = [], []
        for _ in range(reps):
            st = nart_amd.RenderStats()
            r.render(p, st)
            plain_splat.append(st.splat_ms)
            kernel.append(st.kernel_ms)
        res[name] = {"plain_render_splat_ms": med(plain_splat), "plain_render_splat_ms_all": plain_splat,
                     "kernel_ms": med(kernel), "schedule": st.schedule_names()}
        if a.plain_only:
            continue
        K = nart_amd.CascadeParams.defaults().layers
        r.render_robust(p)  # warm-up
        splat, cascade, reweight = [], [], []
        for _ in range(reps):
            st = nart_amd.RenderStats()
            out = r.render_robust(p, stats=st)
            splat.append(st.splat_ms)
            cascade.append(out["cascade_ms"])
            reweight.append(out["reweight_ms"])
        res[name].update({"layers": K, "splat_ms": med(splat), "cascade_ms": med(cascade), "reweight_ms": med(reweight),
                          "cascade_ms_all": cascade, "reweight_ms_all": reweight, "splat_ms_all": splat,
                          "cascade_over_splat": med(cascade) / med(splat),
                          "cascade_over_K_splats": med(cascade) / (K * med(splat))})
    if not a.plain_only:
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, 4
        r.render_denoised(p, beauty=False)  # warm-up
        res["denoise_ms_1080p"] = med(r.render_denoised(p, beauty=False)["denoise_ms"] for _ in range(a.reps))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
