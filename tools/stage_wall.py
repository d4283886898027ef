"""Wall time of one call of every entry point that runs a stage over whole images (render_ms of the
call's nart_render_stats where it has one, the Python call's clock otherwise), glassSphere 1920x1080 /
4 spp: what a change of the host code around the stages can move while the kernels stay the same.
Run it on two builds (NART_HIP_LIB) in one session.  Prints one JSON line of {call: {median, min,
max}} in ms; a development aid, not the bench contract."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import nart_amd  # noqa: E402
from nart_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    path = scenes.glass_sphere()
    r = nart_amd.HipRenderer(nart_amd.Scene(path))
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = 1920, 1080, 4
    aov = r.render_aovs(p, moment=True)
    robust = r.render_robust(p, with_beauty=True, with_layers=True)
    mattes = r.render_mattes(p, with_planes=True)
    gp = nart_amd.GuideParams.defaults()
    with_stats = {
        "render_aovs": lambda st: r.render_aovs(p, stats=st),
        "render_moment": lambda st: r.render_aovs(p, moment=True, stats=st),
        "render_guides": lambda st: r.render_guides(p, gp, stats=st),
        "render_denoised": lambda st: r.render_denoised(p, beauty=False, stats=st),
        "render_denoised_moment": lambda st: r.render_denoised(p, beauty=False, sample_variance=True, stats=st),
        "render_denoised_guides": lambda st: r.render_denoised(p, beauty=False, guides=gp, stats=st),
        "render_adaptive": lambda st: r.render_adaptive(p, stats=st),
        "render_robust": lambda st: r.render_robust(p, stats=st),
        "render_mattes": lambda st: r.render_mattes(p, stats=st),
    }
    host_only = {
        "denoise": lambda: r.denoise(p, aov["beauty"], aov["albedo"], aov["normal"]),
        "denoise_moment": lambda: r.denoise(p, aov["beauty"], aov["albedo"], aov["normal"], moment=aov["moment"]),
        "cascade_reweight": lambda: r.cascade_reweight(p, robust["beauty"], robust["layers"]),
        "matte_rank": lambda: r.matte_rank(p, mattes["planes"], mattes["n_ids"]),
        "matte_extract": lambda: r.matte_extract(p, mattes["ranks"], [0]),
    }
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree"), "frame": "1920x1080, 4 spp", "reps": a.reps}
    for name, call in with_stats.items():
        call(nart_amd.RenderStats())  # warm-up
        ms = []
        for _ in range(a.reps):
            st = nart_amd.RenderStats()
            call(st)
            ms.append(st.render_ms)
        res[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    for name, call in host_only.items():
        call()  # warm-up
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
