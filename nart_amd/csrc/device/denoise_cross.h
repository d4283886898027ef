// Cross-filtered a-trous denoiser over two half buffers (include/nart_hip.h, "Cross-filtered denoising",
// nart_hip_denoise_cross): each half is filtered with colour weights taken from the other half, the
// two results are averaged, and their difference is the error estimate.
//
// Four kernels, one lane per cropped-image pixel, lanes along x, 32 x 8 pixel tiles (256 threads), no
// atomics: every output is a pure function of its inputs, whatever the launch shape.
//   k_dnx_prepare   the five nart_pixel images -> guide {n.xyz, z}, cov, centre {a_d.rgb, alpha}, depth
//                   slope (all as k_dn_prepare computes them) and the two signals {s_h.rgb, v}
//   k_dnx_variance  7x7 guide-weighted mean of v into both signals' v
//   k_dnx_atrous    one 5x5 pass with holes (step 2^i) over both halves, signal ping-pong; the guide
//                   half of a tap weight (dn_tap_guide) is computed once per tap for both halves
//   k_dnx_finalize  average, remodulate and the error image, into totalW x totalH nart_pixel outputs
// The tile view is denoise.h's DnTile<R, 2>: the variance window and the passes of step 1 and 2 stage
// their tile plus halo in LDS (R = 3, 2, 4 pixels of halo); a staged pixel holds two float4 signals, one
// float4 guide and one coverage float, 52 B, at most 40 x 16 pixels = 32.5 KB.  Larger steps read global
// memory (R = 0).  Both ways run the same arithmetic in the same order.
//
// The arithmetic is float32 + - * / sqrt and comparisons only, in the order the header fixes, built
// without contraction: tests/denoise_cross_py.py restates it in numpy and the images agree bit for
// bit.  dn_guides, dn_slope, dn_tap_guide, dn_tap_falloff, dn_window_weight, dn_blur_variance, DnSums and
// dn_remodulate are denoise.h's.
#pragma once

#include "denoise.h"

namespace nd {

struct DnxArgs : DnFilterArgs {
    // inputs / outputs: nart_pixel images of totalW x totalH, 5 floats per pixel
    const float* half[2];
    const float* beauty;
    const float* albedo;
    const float* normal;
    float* out;
    float* error;  // null: no error image
    // work buffers over the cropped W x H image
    float4* guide;  // {n.xyz, z}; an empty pixel is all zeros (z == 0 marks it)
    float* cov;
    const float4* sig_in[2];  // per half {s.rgb, v}; v < 0 marks an invalid pixel (s = 0)
    float4* sig_out[2];
    float4* centre;  // {a_d.rgb, alpha}
    float* slope;
};

__global__ void __launch_bounds__(256) k_dnx_prepare(DnxArgs a) {
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    float c[4];
    dn_mean(a.beauty + p.ti * 5, c);
    float4 g, ce;
    float cov;
    dn_guides(a, p.ti, g, cov, ce);
    ce.w = c[3];
    // the halves' means, each normalised by its own weight sum
    float ch[2][4];
    bool valid = true;
    for (int h = 0; h < 2; ++h) {
        const float* P = a.half[h] + p.ti * 5;
        ch[h][0] = ch[h][1] = ch[h][2] = ch[h][3] = 0.f;
        if (P[3] > 0.f) {
            for (int k = 0; k < 3; ++k) ch[h][k] = P[k] / P[3];
        } else {
            valid = false;
        }
        valid = valid && dn_valid(ch[h]);
    }
    float4 s0 = dn_invalid_signal(), s1 = dn_invalid_signal();
    if (valid) {
        s0 = dn_signal(ch[0], ce, 0.f);
        s1 = dn_signal(ch[1], ce, 0.f);
        const float d = dn_lum(s0) - dn_lum(s1);
        const float v = 0.5f * (d * d);
        s0.w = v;
        s1.w = v;
    }
    const float slope = dn_slope(a, p.x, p.y, p.ti, g.w);
    a.guide[p.i] = g;
    a.cov[p.i] = cov;
    a.sig_out[0][p.i] = s0;
    a.sig_out[1][p.i] = s1;
    a.centre[p.i] = ce;
    a.slope[p.i] = slope;
}

// v <- sum u v / sum u over the 7x7 window's valid taps, u the guide-only tap weight (d_l = 0), the
// centre's 1.  Prepare leaves both halves with one v and one validity, so half 0's is read and the
// result goes to both.
__global__ void __launch_bounds__(256) k_dnx_variance(DnxArgs a) {
    constexpr int R = 3;
    using Tile = DnTile<R, 2, DnxArgs>;
    __shared__ Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y;
    float4 s0 = v.sig(0, x, y), s1 = v.sig(1, x, y);
    if (s0.w < 0.f) {  // invalid: stays as it is
        a.sig_out[0][p.i] = s0;
        a.sig_out[1][p.i] = s1;
        return;
    }
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    float su = 0.f, sv = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)a.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)a.W) continue;
            const float vq = v.sig(0, qx, qy).w;
            if (vq < 0.f) continue;
            const float u = dn_window_weight(a, v, gp, covp, slope_p, dx, dy, qx, qy);
            su = su + u;
            sv = sv + u * vq;
        }
    }
    const float vp = sv / su;
    s0.w = vp;
    s1.w = vp;
    a.sig_out[0][p.i] = s0;
    a.sig_out[1][p.i] = s1;
}

template <int R>
__global__ void __launch_bounds__(256) k_dnx_atrous(DnxArgs a) {
    using Tile = DnTile<R, 2, DnxArgs>;
    __shared__ typename Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y, W = (int)a.W, H = (int)a.H;
    const int step = (int)a.step;
    const float4 sp[2] = {v.sig(0, x, y), v.sig(1, x, y)};
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    // vp[h]: half h is valid at the centre.  Half h's colour distances are the other half's: they are
    // taken where the other half is valid at the centre, against den[h] from the 3x3 blur of the other
    // half's variance
    const bool vp[2] = {!(sp[0].w < 0.f), !(sp[1].w < 0.f)};
    float den[2] = {0.f, 0.f}, lp[2] = {0.f, 0.f};
    if (vp[0] || vp[1]) {
        const float vb[2] = {dn_blur_variance(v, 0, x, y, W, H), dn_blur_variance(v, 1, x, y, W, H)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int o = 1 - h;
            if (vp[o]) {
                den[h] = a.sigma_color * sqrtf(vb[o]) + 1e-6f;
                lp[h] = dn_lum(sp[o]);
            }
        }
    }
    DnSums sum[2];
    for (int iy = -2; iy <= 2; ++iy) {
        const int qy = y + iy * step;
        if (qy < 0 || qy >= H) continue;
        const float hy = dn_tap5(iy);
        for (int ix = -2; ix <= 2; ++ix) {
            const int qx = x + ix * step;
            if (qx < 0 || qx >= W) continue;
            const float4 sq[2] = {v.sig(0, qx, qy), v.sig(1, qx, qy)};
            const bool vq[2] = {!(sq[0].w < 0.f), !(sq[1].w < 0.f)};
            if (!vq[0] && !vq[1]) continue;
            const float hx = dn_tap5(ix);
            const bool centre = ix == 0 && iy == 0;
            float wn = 1.f, dg = 0.f;
            if (!centre) {
                const int cheb = step * max(abs(ix), abs(iy));
                dn_tap_guide(a, gp, covp, slope_p, v.guide(qx, qy), v.cov(qx, qy), (float)cheb, wn, dg);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (!vq[h]) continue;
                float w = hx * hy;
                if (!centre) {
                    const int o = 1 - h;
                    const float d_l = vp[o] && vq[o] ? dn_abs(lp[h] - dn_lum(sq[o])) / den[h] : 0.f;
                    w = w * dn_tap_falloff(wn, dg, d_l);
                }
                sum[h].add(w, sq[h]);
            }
        }
    }
    a.sig_out[0][p.i] = sum[0].result();
    a.sig_out[1][p.i] = sum[1].result();
}

// Average and remodulate: cropped pixels {((s_0 + s_1) * 0.5) * a_d, alpha, 1} and, in the error image,
// {t * t per channel, alpha, 1} with t = ((s_0 - s_1) * 0.5) * a_d; a pixel with an invalid half gets the
// beauty's mean and error 0; border pixels zero (sig_in: the last pass's output).
__global__ void __launch_bounds__(256) k_dnx_finalize(DnxArgs a) {
    const size_t n = (size_t)a.totalW * a.totalH;
    const size_t ti = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ti >= n) return;
    size_t i;
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, e[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (dn_cropped(a, ti, i)) {
        const float4 s0 = a.sig_in[0][i], s1 = a.sig_in[1][i], ce = a.centre[i];
        if (s0.w < 0.f || s1.w < 0.f) {
            float c[4];
            dn_mean(a.beauty + ti * 5, c);
            o[0] = c[0];
            o[1] = c[1];
            o[2] = c[2];
        } else {
            const float4 mean = make_float4((s0.x + s1.x) * 0.5f, (s0.y + s1.y) * 0.5f, (s0.z + s1.z) * 0.5f, 0.f);
            const float4 diff = make_float4((s0.x - s1.x) * 0.5f, (s0.y - s1.y) * 0.5f, (s0.z - s1.z) * 0.5f, 0.f);
            float t[5];
            dn_remodulate(mean, ce, ce.w, o);
            dn_remodulate(diff, ce, ce.w, t);
            e[0] = t[0] * t[0];
            e[1] = t[1] * t[1];
            e[2] = t[2] * t[2];
        }
        o[3] = e[3] = ce.w;
        o[4] = e[4] = 1.f;
    }
    dn_store_pixel(a.out, ti, o);
    if (a.error) dn_store_pixel(a.error, ti, e);
}

}  // namespace nd
