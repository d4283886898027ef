"""What the parts denoise (nart_hip_denoise_parts, nart_hip_render_denoised_light_groups) costs next to
what a user could do before it: the measurements A and B of DESIGN.md, "Denoised parts".

A. The fused stage against K runs of the denoiser, device time (the kernels' events), on the same images:
   the K parts are the two light groups of the materials scene at 1920x1080, repeated with other gains.
   Yardstick: nart_hip_denoise once per part, its kernel times (nart_hip_denoise_timings) summed.  Against
   it: nart_hip_denoise_parts' kernel times (nart_hip_denoise_parts_timings, no sum asked for) with the
   chunk size forced to 1..4 (NART_DN_PARTS_CHUNK) and on the automatic plan.  The sides alternate within
   every repetition; medians of --reps after one warm-up round; spread = (max - min) / median.  In the
   warm-up round every fused output is compared with the separate run's, bit for bit, at the timed size.
B. The whole call, wall time: render_light_groups + render_aovs(beauty=False) + one host denoise per group
   against render_denoised_light_groups, and the guides frame's render_ms over the group frame's.

Prints one JSON line per measurement; a development aid, not the bench contract."""
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

med = statistics.median


def spread(v):
    return (max(v) - min(v)) / med(v) if med(v) else 0.0


def dn_total(t):
    return t["prepare"] + t["variance"] + sum(t["passes"]) + t["finalize"]


def stage_a(r, p, parts2, aov, Ks, reps):
    for K in Ks:
        parts = np.stack([parts2[k % 2] * np.float32(1.0 + 0.125 * k) for k in range(K)])
        sides = ["separate", "auto", "1", "2", "3", "4"]
        ms = {s: [] for s in sides}
        split = {s: [] for s in sides}
        for rep in range(reps + 1):
            for s in sides:
                if s == "separate":
                    t = 0.0
                    alone = []
                    for k in range(K):
                        alone.append(r.denoise(p, parts[k], aov["albedo"], aov["normal"]))
                        t += dn_total(r.denoise_timings())
                    tm = None
                else:
                    if s == "auto":
                        os.environ.pop("NART_DN_PARTS_CHUNK", None)
                    else:
                        os.environ["NART_DN_PARTS_CHUNK"] = s
                    fused = r.denoise_parts(p, parts, aov["albedo"], aov["normal"])
                    tm = r.denoise_parts_timings()
                    if not rep:  # faster and different is not faster: the bits at the size that is timed
                        same = all(np.array_equal(fused[k].view(np.uint32), alone[k].view(np.uint32)) for k in range(K))
                        assert same, "K = %d, chunk %s: the fused stage differs from the separate runs" % (K, s)
                    t = dn_total(tm)
                if rep:  # (round 0 warms up)
                    ms[s].append(t)
                    split[s].append(tm)
        os.environ.pop("NART_DN_PARTS_CHUNK", None)
        res = {"measurement": "A", "K": K, "bits_equal_to_separate": True, "width": p.image_width, "height": p.image_height, "reps": reps}
        for s in sides:
            res[s] = {"ms": med(ms[s]), "spread": spread(ms[s]), "all": ms[s]}
            if s != "separate":
                res[s]["over_separate"] = med(ms[s]) / med(ms["separate"])
                res[s]["prepare"] = med(x["prepare"] for x in split[s])
                res[s]["variance"] = med(x["variance"] for x in split[s])
                res[s]["passes"] = [med(x["passes"][i] for x in split[s]) for i in range(8)]
                res[s]["finalize"] = med(x["finalize"] for x in split[s])
        print(json.dumps(res), flush=True)


def stage_b(r, p, groups, reps):
    G = max(groups) + 1
    old, new, ratio, dn_ms = [], [], [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        st = nart_amd.RenderStats()
        lg = r.render_light_groups(p, groups, stats=st)
        aov = r.render_aovs(p, beauty=False)
        for g in range(G):
            r.denoise(p, lg["groups"][g], aov["albedo"], aov["normal"])
        t1 = time.perf_counter()
        out = r.render_denoised_light_groups(p, groups, with_sum=False)
        t2 = time.perf_counter()
        if rep:
            old.append((t1 - t0) * 1e3)
            new.append((t2 - t1) * 1e3)
            ratio.append(out["guides_ms"] / st.render_ms)
            dn_ms.append(out["denoise_ms"])
    print(json.dumps({"measurement": "B", "groups": G, "width": p.image_width, "height": p.image_height, "spp": p.spp,
                      "reps": reps, "separate_wall_ms": med(old), "separate_spread": spread(old), "separate_all": old,
                      "fused_wall_ms": med(new), "fused_spread": spread(new), "fused_all": new,
                      "fused_over_separate": med(new) / med(old), "guides_frame_over_group_frame": med(ratio),
                      "denoise_ms": med(dn_ms)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-w", type=int, default=1920)
    ap.add_argument("-H", type=int, default=1080)
    ap.add_argument("-s", type=int, default=16, help="samples per pixel of measurement B")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="2,3,4,8,9")
    ap.add_argument("--only", default="AB")
    a = ap.parse_args()
    path = scenes.materials()
    scene = nart_amd.Scene(path)
    p = nart_amd.load_sessions(path)[0]
    p.image_width, p.image_height, p.spp = a.w, a.H, 4
    r = nart_amd.HipRenderer(scene)
    if "A" in a.only:
        lg = r.render_light_groups(p, [0, 1])
        aov = r.render_aovs(p, beauty=False)
        stage_a(r, p, lg["groups"], aov, [int(k) for k in a.parts.split(",")], a.reps)
    if "B" in a.only:
        p.spp = a.s
        stage_b(r, p, [0, 1], a.reps)
    r.close()


if __name__ == "__main__":
    main()
