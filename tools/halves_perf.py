"""Cost of the half buffers and the cross-filtered denoiser at 1920x1080 (cornell), one context, the median
of --reps after a warm-up of each:
  render      render_ms (wall) and device_ms (LatinSquare, path kernels, splat: HIP events) of a plain render
              at --spp; with this build also render_halves (the two
              split-and-splat passes: halves_ms is their device time) and their ratio;
  denoise     device time (denoise_ms, HIP events) of the plain denoise() over the beauty of a 4-spp
              render and its first-hit AOVs, twice; with this build also denoise_cross over the two
              halves of the same render, its kernels one by one, and its ratio to two denoise() calls.
--parent measures the plain render and denoise() alone: run it on the parent's build (NART_HIP_LIB) in
the same session, alternating, for the parent's figures.  The inputs of the denoisers are rendered by the
build under test; the plain kernels are the same code in both.  Prints one JSON line; a development aid,
not the bench contract."""
import argparse
import ctypes
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
    res = {"build": os.environ.get("NART_HIP_LIB", "in-tree"), "frame": "%dx%d" % (a.width, a.height), "reps": a.reps}
    path = scenes.cornell()
    scene = nart_amd.Scene(path)
    r = nart_amd.HipRenderer(scene)
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = a.width, a.height, a.spp

    def measure(call):
        call()  # warm-up
        t = [call() for _ in range(a.reps)]
        return {"ms": med(t), "all": [round(x, 3) for x in t]}

    kernel_ms = []

    def render_ms(fn):
        def once():
            st = nart_amd.RenderStats()
            fn(st)
            kernel_ms.append(st.kernel_ms + st.splat_ms + st.latin_ms)
            return st.render_ms
        return once

    out = res["render_%dspp" % a.spp] = {"render": measure(render_ms(lambda st: r.render(p, stats=st)))}
    out["render"]["device_ms"] = med(kernel_ms[1:])  # LatinSquare, path kernels and the beauty's splat (HIP events)
    if not a.parent:
        halves_ms = []

        def halves(st):
            halves_ms.append(r.render_halves(p, stats=st)["halves_ms"])
        out["render_halves"] = measure(render_ms(halves))
        out["halves_ms"] = med(halves_ms[1:])
        out["ratio"] = out["render_halves"]["ms"] / out["render"]["ms"]
        out["added_ms"] = out["render_halves"]["ms"] - out["render"]["ms"]

    p4 = nart_amd.load_sessions(path)[0]
    p4.image_width, p4.image_height, p4.spp = a.width, a.height, 4
    aov = r.render_aovs(p4)
    lib, ms = nart_amd.hip_lib(), ctypes.c_double()
    dst = aov["beauty"].copy()

    def plain():
        r._check(lib.nart_hip_denoise(r._ctx, ctypes.byref(p4), None, aov["beauty"].ctypes.data, aov["albedo"].ctypes.data,
                                      aov["normal"].ctypes.data, dst.ctypes.data, ctypes.byref(ms)))
        return ms.value
    d = res["denoise"] = {"denoise": measure(plain)}
    d["denoise_kernels"] = r.denoise_timings()
    d["two_denoise_ms"] = 2 * d["denoise"]["ms"]
    if not a.parent:
        h = r.render_halves(p4)
        images = (h["halves"][0], h["halves"][1], aov["beauty"], aov["albedo"], aov["normal"])
        d["denoise_cross"] = measure(lambda: r.denoise_cross(p4, *images)["denoise_ms"])
        d["denoise_cross_kernels"] = r.denoise_cross_timings()
        d["ratio_to_two_denoise"] = d["denoise_cross"]["ms"] / d["two_denoise_ms"]
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
