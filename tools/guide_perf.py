"""Cost and quality of the followed guides next to the first-hit AOVs they replace.

Cost: guide_ms (k_guide + the two guide splats) against aov_ms (k_aov twice + the two AOV splats) of
the same glassSphere 1920x1080 frame, at 4 spp and on the C3 frame (256 spp), medians and ranges after
a warm-up; and render_denoised's wall time and denoise_ms with and without guides at 4 spp.
Quality (--quality): DESIGN.md's test C -- 128x128, 4 spp against 512 spp of the same renderer,
relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) over the pixels whose 512-spp first-hit coverage is >=
0.999 -- on glassSphere and `materials`: noisy, denoised with first-hit guides, denoised with followed
guides, in the spatial and the sample-variance mode.
Prints one JSON line; a development aid, not the bench contract."""
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
from nart_amd import GuideParams, scenes  # noqa: E402


def _stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def cost(a):
    path = scenes.glass_sphere()
    scene = nart_amd.Scene(path)
    r = nart_amd.HipRenderer(scene)
    gp = GuideParams.defaults(max_follow=a.max_follow)
    res = {}
    for name, spp, reps in (("1080p_4spp", 4, a.reps), ("c3", 256, a.c3_reps)):
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, spp
        r.render_aovs(p)  # warm-up
        r.render_guides(p, gp)
        aov, guide, kernel = [], [], []
        for _ in range(reps):
            st = nart_amd.RenderStats()
            aov.append(r.render_aovs(p, stats=st)["aov_ms"])
            kernel.append(st.kernel_ms)
            guide.append(r.render_guides(p, gp)["guide_ms"])
        res[name] = {"aov_ms": _stat(aov), "guide_ms": _stat(guide), "kernel_ms": _stat(kernel),
                     "guide_over_aov": statistics.median(guide) / statistics.median(aov)}
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = 1920, 1080, 4
    for mode, guides in (("first_hit", None), ("followed", gp)):
        r.render_denoised(p, beauty=False, guides=guides)  # warm-up
        wall, dn = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dn.append(r.render_denoised(p, beauty=False, guides=guides)["denoise_ms"])
            wall.append((time.perf_counter() - t0) * 1e3)
        res["render_denoised_" + mode] = {"wall_ms": _stat(wall), "denoise_ms": _stat(dn)}
    return res


def quality(a):
    import tempfile
    res = {}
    gp = GuideParams.defaults(max_follow=a.max_follow)
    for name, path in (("glassSphere", scenes.glass_sphere()), ("materials", scenes.materials(tempfile.mkdtemp()))):
        scene = nart_amd.Scene(path)
        r = nart_amd.HipRenderer(scene)
        p4, p512 = nart_amd.load_sessions(path)[0], nart_amd.load_sessions(path)[0]
        p4.image_width, p4.image_height, p4.spp = 128, 128, 4
        p512.image_width, p512.image_height, p512.spp = 128, 128, 512
        ref = r.render_aovs(p512, normal=False)
        mask = nart_amd.finalize(p512, ref["albedo"])[..., 3] >= 0.999
        x_ref = nart_amd.finalize(p512, ref["beauty"])[..., :3].astype(np.float64)

        def rel_mse(img):
            x = nart_amd.finalize(p4, img)[..., :3].astype(np.float64)
            return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

        row = {"mask_keeps": float(mask.mean())}
        for mode, sv in (("spatial", False), ("sample_variance", True)):
            first = r.render_denoised(p4, sample_variance=sv)
            followed = r.render_denoised(p4, sample_variance=sv, guides=gp)
            row[mode] = {"noisy": rel_mse(first["beauty"]), "first_hit": rel_mse(first["denoised"]),
                         "followed": rel_mse(followed["denoised"])}
        res[name] = row
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--c3-reps", type=int, default=3)
    ap.add_argument("--max-follow", type=int, default=8)
    ap.add_argument("--quality", action="store_true", help="the relMSE table instead of the timings")
    a = ap.parse_args()
    print(json.dumps(quality(a) if a.quality else cost(a)), flush=True)


if __name__ == "__main__":
    main()
