"""Cost of the second-moment image and of the sample-variance denoiser next to what they sit beside:
moment_ms (k_moment + the moment splat) and splat_ms (the beauty's splat + combine) of the same
frames, at 1920x1080 / 4 spp and on the C3 frame (glassSphere 1920x1080, 256 spp), and denoise_ms of
both variance modes at 1920x1080 / 4 spp, kernel by kernel.  Prints one JSON line; a development
aid, not the bench contract."""
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
    a = ap.parse_args()
    path = scenes.glass_sphere()
    scene = nart_amd.Scene(path)
    r = nart_amd.HipRenderer(scene)
    med = statistics.median
    res = {}
    for name, spp, reps in (("1080p_4spp", 4, a.reps), ("c3", 256, a.c3_reps)):
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = 1920, 1080, spp
        r.render_aovs(p, albedo=False, normal=False, moment=True)  # warm-up
        splat, moment, kernel, plain_splat = [], [], [], []
        for _ in range(reps):
            st = nart_amd.RenderStats()
            out = r.render_aovs(p, albedo=False, normal=False, moment=True, stats=st)
            splat.append(st.splat_ms)
            kernel.append(st.kernel_ms)
            moment.append(out["moment_ms"])
            st = nart_amd.RenderStats()
            r.render(p, st)
            plain_splat.append(st.splat_ms)
        res[name] = {"splat_ms": med(splat), "moment_ms": med(moment), "moment_ms_all": moment, "splat_ms_all": splat,
                     "kernel_ms": med(kernel), "plain_render_splat_ms": med(plain_splat),
                     "moment_over_splat": med(moment) / med(splat), "schedule": st.schedule_names()}
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = 1920, 1080, 4
    for mode, sv in (("spatial", False), ("sample_variance", True)):
        r.render_denoised(p, beauty=False, sample_variance=sv)  # warm-up
        dn, split = [], []
        for _ in range(a.reps):
            dn.append(r.render_denoised(p, beauty=False, sample_variance=sv)["denoise_ms"])
            split.append(r.denoise_timings())
        res["denoise_" + mode] = {"denoise_ms": med(dn), "denoise_ms_all": dn,
                                  "prepare_ms": med(s["prepare"] for s in split),
                                  "variance_ms": med(s["variance"] for s in split),
                                  "pass_ms": [med(s["passes"][i] for s in split) for i in range(5)],
                                  "finalize_ms": med(s["finalize"] for s in split)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
