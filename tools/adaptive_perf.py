"""Cost and yield of adaptive sampling (HipRenderer.render_adaptive) on the C3 frame (glassSphere
1920x1080, max 256 spp) and the C2 frame (Cornell box 1920x1080, max 64 spp), next to the uniform
render of the same process: wall ms and samples taken of both, the buckets rendered per level,
adaptive_ms (the error and scatter kernels) as a share of the call, and the quantiles of the pilot
pass's bucket errors, which place a threshold.  --thresholds sweeps further thresholds beside the
default.  Prints one JSON line; a development aid, not the bench contract."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nart_amd  # noqa: E402
from nart_amd import scenes  # noqa: E402


def timed(call, reps):
    ms, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--thresholds", default="", help="comma-separated thresholds to run beside the default")
    ap.add_argument("--configs", default="c3,c2")
    a = ap.parse_args()
    default = nart_amd.AdaptiveParams.defaults()
    thresholds = [float(default.threshold)] + [float(t) for t in a.thresholds.split(",") if t]
    res = {"defaults": {"min_spp": default.min_spp, "growth": default.growth, "threshold": float(default.threshold),
                        "floor": float(default.floor)}}
    for name, make, spp in (("c3", scenes.glass_sphere, 256), ("c2", scenes.cornell, 64)):
        if name not in a.configs.split(","):
            continue
        path = make()
        r = nart_amd.HipRenderer(nart_amd.Scene(path))
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, spp
        r.render(p)  # warm-up
        st = nart_amd.RenderStats()
        ms, all_ms, _ = timed(lambda: r.render(p, st), a.reps)
        cfg = {"uniform": {"wall_ms": ms, "wall_ms_all": all_ms, "samples": st.samples // a.reps}}
        pilot = r.render_adaptive(p, nart_amd.AdaptiveParams.defaults(threshold=float("inf")))
        E = pilot["bucket_error"].reshape(-1).astype(np.float64)
        cfg["pilot_error_quantiles"] = {q: float(np.quantile(E, q)) for q in (0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)}
        cfg["pilot_error_zero_share"] = float((E == 0).mean())
        for thr in thresholds:
            params = nart_amd.AdaptiveParams.defaults(threshold=thr)
            r.render_adaptive(p, params)  # warm-up
            ad_ms, samples = [], 0
            ms, all_ms, out = timed(lambda: r.render_adaptive(p, params), a.reps)
            for _ in range(a.reps):
                st = nart_amd.RenderStats()
                o = r.render_adaptive(p, params, stats=st)
                ad_ms.append(o["adaptive_ms"])
                samples = st.samples
            spp_b = out["bucket_spp"].reshape(-1)
            cfg["threshold_%g" % thr] = {
                "wall_ms": ms, "wall_ms_all": all_ms, "samples": int(samples), "levels": out["levels"],
                "buckets_rendered_per_level": [int((spp_b >= L).sum()) for L in out["levels"]],
                "adaptive_ms": statistics.median(ad_ms), "adaptive_share": statistics.median(ad_ms) / ms,
                "samples_over_uniform": samples / float(cfg["uniform"]["samples"]),
                "wall_over_uniform": ms / cfg["uniform"]["wall_ms"]}
        r.close()
        res[name] = cfg
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
