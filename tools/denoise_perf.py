"""Cost of the a-trous denoiser (nart_hip_render_denoised) next to the render it cleans: device
time of the denoise at 1920x1080 with the default parameters, kernel by kernel
(nart_hip_denoise_timings), the must-move bandwidth of the a-trous passes (36 B read + 16 B written
per pixel per pass over the pass time), and render_ms of the plain render() of the same frame -- a
path this feature leaves as it was -- for scale.  Prints one JSON line; a development aid, not the
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
    ap.add_argument("--scene", default="glass", choices=["glass", "cornell"])
    ap.add_argument("-w", type=int, default=1920)
    ap.add_argument("-H", type=int, default=1080)
    ap.add_argument("-s", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=0, help="a-trous passes (0: the default)")
    a = ap.parse_args()
    path = scenes.glass_sphere() if a.scene == "glass" else scenes.cornell()
    scene = nart_amd.Scene(path)
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = a.w, a.H, a.s
    dp = nart_amd.DenoiseParams.defaults()
    if a.iterations:
        dp.iterations = a.iterations
    r = nart_amd.HipRenderer(scene)
    r.render_denoised(p, dp, beauty=False)  # warm-up: allocations, code upload
    r.render(p)
    render_ms, denoised_ms, dn_ms, split = [], [], [], []
    for _ in range(a.reps):
        st = nart_amd.RenderStats()
        r.render(p, st)
        render_ms.append(st.render_ms)
        st = nart_amd.RenderStats()
        out = r.render_denoised(p, dp, beauty=False, stats=st)
        denoised_ms.append(st.render_ms)
        dn_ms.append(out["denoise_ms"])
        split.append(r.denoise_timings())
    med = statistics.median
    npx = a.w * a.H
    passes = [med(s["passes"][i] for s in split) for i in range(dp.iterations)]
    res = {
        "scene": a.scene, "width": a.w, "height": a.H, "spp": a.s, "reps": a.reps, "iterations": dp.iterations,
        "render_ms": med(render_ms), "render_ms_all": render_ms,
        "render_denoised_ms": med(denoised_ms),
        "denoise_ms": med(dn_ms), "denoise_ms_all": dn_ms,
        "prepare_ms": med(s["prepare"] for s in split), "variance_ms": med(s["variance"] for s in split),
        "pass_ms": passes, "finalize_ms": med(s["finalize"] for s in split),
        # must-move: {guide 16, signal 16, cov 4} read and a 16 B signal record written per pixel
        "pass_must_move_gb_s": [npx * 52 / (t * 1e-3) / 1e9 for t in passes],
        "denoise_over_render": med(dn_ms) / med(render_ms),
    }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
