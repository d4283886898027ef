"""The cross-filtered denoiser's quality figures on the CPU, before any device runs it: Cornell at
--size x --size, --spp samples, against an oracle render at --ref-spp, with tests/test_gpu_denoise_cross.py's
relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) and mask (first-hit coverage >= 0.999).  Everything comes from
the CPU restatements: the beauty and the half buffers are splatted from the oracle's per-sample Li_alpha
(tests/halves_py.py), the first-hit albedo and normal images from the oracle's camera-ray hits (the
material's constant pattern, the float32 shading normal and the hit distance, per sample, splatted the same
way), the plain filter is tests/denoise_py.py and the cross filter tests/denoise_cross_py.py.  Prints one
JSON line: relMSE of the noisy, plain-denoised and cross-denoised images, the ratios, and the correlation
of the error image with the true squared error after a 5 x 5 box blur of both.  A development aid."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, d)

import nart_amd  # noqa: E402
import oracle  # noqa: E402
from nart_amd import scenes  # noqa: E402

import aov_py  # noqa: E402
import denoise_cross_py as dx  # noqa: E402
import denoise_py as dn  # noqa: E402
import halves_py as hp  # noqa: E402
from test_aov_restatement import restate_render  # noqa: E402

f32 = np.float32


def box5(a):
    H, W = a.shape[:2]
    pad = np.pad(a, ((2, 2), (2, 2)), mode="edge")
    out = np.zeros((H, W))
    for dy in range(5):
        for dx_ in range(5):
            out += pad[dy:dy + H, dx_:dx_ + W]
    return out / 25.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=512)
    a = ap.parse_args()
    from nart_amd import build as nb
    nb.build_scene_lib()
    oracle.build()
    path = scenes.cornell()
    scene = nart_amd.Scene(path)
    orc = oracle.Oracle(scene)

    def params(spp):
        p = nart_amd.load_sessions(path)[0]
        p.image_width, p.image_height, p.spp = a.size, a.size, spp
        return p

    p, pref = params(a.spp), params(a.ref_spp)
    g = nart_amd.session_geometry(p)
    W = H = a.size
    fb = g.filter_bounds
    L, uv = orc.render_samples(p, 0, 0, g.total_width, g.total_height, with_uv=True)
    beauty = restate_render(p, uv, L)
    halves = hp.restate_halves(p, uv, L)
    # first-hit records per sample from the oracle's camera-ray hits
    ref = aov_py.trace_block(orc, p, 0, 0, g.total_width, g.total_height)
    mats, tri_mat, tris = scene.materials(), aov_py.tri_material(scene), scene.triangles()
    alb = np.zeros(L.shape, f32)
    nrm = np.zeros(L.shape, f32)
    # a camera ray that meets a disk light before the surface is a miss for the first-hit AOVs (the octree
    # holds no lights): row-major transforms, the disk in its local z = 0 plane
    with open(path) as fh:
        disks = [l for l in json.load(fh)["lights"] if l["type"] == "disk"]
    o64, d64 = ref["o"].astype(np.float64), ref["d"].astype(np.float64)
    lit = np.zeros(ref["tri"].shape, bool)
    for l in disks:
        m = np.array(l["transform"], np.float64).reshape(4, 4)
        c, n = m[:3, 3], m[:3, 2]
        with np.errstate(all="ignore"):
            t = ((c - o64) @ n) / (d64 @ n)
            hit = o64 + t[..., None] * d64
            near = np.where(ref["tri"] >= 0, ref["t"].astype(np.float64), np.inf)
            lit |= (t > 0) & (t < near) & (((hit - c) ** 2).sum(-1) <= l["radius"] ** 2)
    for idx in zip(*np.nonzero((ref["tri"] >= 0) & ~lit)):
        t = ref["tri"][idx]
        ptn = aov_py.albedo_pattern(mats[tri_mat[t]])
        alb[idx][:3] = f32(list(ptn.value))
        alb[idx][3] = 1
        nrm[idx][:3] = aov_py.shading_normal(tris[t], ref["o"][idx], ref["d"][idx], np.float32)
        nrm[idx][3] = ref["t"][idx]
    albedo, normal = restate_render(p, uv, alb), restate_render(p, uv, nrm)
    x_ref = nart_amd.finalize(pref, orc.render(pref))[..., :3].astype(np.float64)
    mask = nart_amd.finalize(p, albedo)[..., 3] >= 0.999
    plain = dn.denoise(W, H, fb, beauty, albedo, normal)
    cross, err = dx.denoise(W, H, fb, halves[0], halves[1], beauty, albedo, normal)

    def rel_mse(img):
        x = nart_amd.finalize(p, img)[..., :3].astype(np.float64)
        return float((((x - x_ref) ** 2) / (x_ref ** 2 + 0.01))[mask].mean())

    noisy, den, crs = rel_mse(beauty), rel_mse(plain), rel_mse(cross)
    true_sq = ((nart_amd.finalize(p, cross)[..., :3].astype(np.float64) - x_ref) ** 2).mean(-1)
    est = nart_amd.finalize(p, err)[..., :3].astype(np.float64).mean(-1)
    ta, eb = box5(true_sq)[mask], box5(est)[mask]
    print(json.dumps({"scene": "cornell %dx%d, %d spp against %d spp (oracle)" % (W, H, a.spp, a.ref_spp),
                      "mask_keeps": float(mask.mean()), "relmse_noisy": noisy, "relmse_plain": den, "relmse_cross": crs,
                      "cross_over_noisy": crs / noisy, "cross_over_plain": crs / den, "cross_below_noisy": crs < noisy,
                      "error_correlation_box5": float(np.corrcoef(ta, eb)[0, 1]),
                      "error_mean_over_true_mean": float(eb.mean() / ta.mean())}))


if __name__ == "__main__":
    main()
