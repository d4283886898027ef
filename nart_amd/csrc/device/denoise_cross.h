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
// The LDS halo scheme is denoise.h's: the variance window and the passes of step 1 and 2 stage their
// tile plus halo in LDS (R = 3, 2, 4 pixels of halo); a staged pixel holds two float4 signals, one
// float4 guide and one coverage float, 52 B, at most 40 x 16 pixels = 32.5 KB.  Larger steps read global
// memory (R = 0).  Both ways run the same arithmetic in the same order.
//
// The arithmetic is float32 + - * / sqrt and comparisons only, in the order the header fixes, built
// without contraction: tests/denoise_cross_py.py restates it in numpy and the images agree bit for
// bit.  dn_guides, dn_slope, dn_tap_guide and dn_tap_falloff are denoise.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise.h"

namespace nd {

struct DnxArgs {
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
    uint32_t W, H, totalW, totalH, fb;
    uint32_t step;
    uint32_t normal_squarings;
    float sigma_color, sigma_depth, depth_eps, sigma_coverage, albedo_floor;
};

__global__ void __launch_bounds__(256) k_dnx_prepare(DnxArgs a) {
    const uint32_t x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    const uint32_t y = blockIdx.y * DN_TH + threadIdx.x / DN_TW;
    if (x >= a.W || y >= a.H) return;
    const size_t ti = (size_t)(y + a.fb) * a.totalW + (x + a.fb);
    const size_t i = (size_t)y * a.W + x;
    float c[4];
    dn_mean(a.beauty + ti * 5, c);
    float4 g, ce;
    float cov;
    dn_guides(a, ti, g, cov, ce);
    ce.w = c[3];
    // the halves' means, each normalised by its own weight sum
    float ch[2][4];
    bool valid = true;
    for (int h = 0; h < 2; ++h) {
        const float* P = a.half[h] + ti * 5;
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
    const float slope = dn_slope(a, x, y, ti, g.w);
    a.guide[i] = g;
    a.cov[i] = cov;
    a.sig_out[0][i] = s0;
    a.sig_out[1][i] = s1;
    a.centre[i] = ce;
    a.slope[i] = slope;
}

// A block's view of the per-tap records: its tile plus R pixels of halo in LDS (R > 0), or global
// memory (R == 0).  at() is only called with coordinates inside the image.
template <int R>
struct DnxView {
    static constexpr int LW = DN_TW + 2 * R, LH = DN_TH + 2 * R;
    float4* lg;
    float4* ls0;
    float4* ls1;
    float* lc;
    const DnxArgs& a;
    int x0, y0;  // image coordinates of the staged region's first pixel

    __device__ DnxView(const DnxArgs& args, float4* g, float4* s0, float4* s1, float* c)
        : lg(g), ls0(s0), ls1(s1), lc(c), a(args) {
        x0 = (int)(blockIdx.x * DN_TW) - R;
        y0 = (int)(blockIdx.y * DN_TH) - R;
        if (R > 0) {
            for (int k = threadIdx.x; k < LW * LH; k += 256) {
                const int gx = x0 + k % LW, gy = y0 + k / LW;
                float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f), a4 = make_float4(0.f, 0.f, 0.f, -1.f), b4 = a4;
                float c1 = 0.f;
                if (gx >= 0 && gy >= 0 && gx < (int)a.W && gy < (int)a.H) {
                    const size_t i = (size_t)gy * a.W + gx;
                    g4 = a.guide[i];
                    a4 = a.sig_in[0][i];
                    b4 = a.sig_in[1][i];
                    c1 = a.cov[i];
                }
                lg[k] = g4;
                ls0[k] = a4;
                ls1[k] = b4;
                lc[k] = c1;
            }
            __syncthreads();
        }
    }
    __device__ __forceinline__ size_t idx(int x, int y) const {
        return R > 0 ? (size_t)((y - y0) * LW + (x - x0)) : (size_t)y * a.W + x;
    }
    __device__ __forceinline__ float4 guide(int x, int y) const { return R > 0 ? lg[idx(x, y)] : a.guide[idx(x, y)]; }
    __device__ __forceinline__ float4 sig0(int x, int y) const { return R > 0 ? ls0[idx(x, y)] : a.sig_in[0][idx(x, y)]; }
    __device__ __forceinline__ float4 sig1(int x, int y) const { return R > 0 ? ls1[idx(x, y)] : a.sig_in[1][idx(x, y)]; }
    __device__ __forceinline__ float cov(int x, int y) const { return R > 0 ? lc[idx(x, y)] : a.cov[idx(x, y)]; }
};

// v <- sum u v / sum u over the 7x7 window's valid taps, u the guide-only tap weight (d_l = 0), the
// centre's 1.  Prepare leaves both halves with one v and one validity, so half 0's is read and the
// result goes to both.
__global__ void __launch_bounds__(256) k_dnx_variance(DnxArgs a) {
    constexpr int R = 3;
    constexpr int N = DnxView<R>::LW * DnxView<R>::LH;
    __shared__ float4 lg[N];
    __shared__ float4 ls0[N];
    __shared__ float4 ls1[N];
    __shared__ float lc[N];
    const DnxView<R> v(a, lg, ls0, ls1, lc);
    const int x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int y = blockIdx.y * DN_TH + threadIdx.x / DN_TW;
    if (x >= (int)a.W || y >= (int)a.H) return;
    const size_t i = (size_t)y * a.W + x;
    float4 s0 = v.sig0(x, y), s1 = v.sig1(x, y);
    if (s0.w < 0.f) {  // invalid: stays as it is
        a.sig_out[0][i] = s0;
        a.sig_out[1][i] = s1;
        return;
    }
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[i];
    float su = 0.f, sv = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)a.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)a.W) continue;
            const float vq = v.sig0(qx, qy).w;
            if (vq < 0.f) continue;
            float u = 1.f;
            if (dx != 0 || dy != 0) {
                const int cheb = max(abs(dx), abs(dy));
                float wn, dg;
                dn_tap_guide(a, gp, covp, slope_p, v.guide(qx, qy), v.cov(qx, qy), (float)cheb, wn, dg);
                u = dn_tap_falloff(wn, dg, 0.f);
            }
            su = su + u;
            sv = sv + u * vq;
        }
    }
    const float vp = sv / su;
    s0.w = vp;
    s1.w = vp;
    a.sig_out[0][i] = s0;
    a.sig_out[1][i] = s1;
}

template <int R>
__global__ void __launch_bounds__(256) k_dnx_atrous(DnxArgs a) {
    constexpr int N = R > 0 ? DnxView<R>::LW * DnxView<R>::LH : 1;
    __shared__ float4 lg[N];
    __shared__ float4 ls0[N];
    __shared__ float4 ls1[N];
    __shared__ float lc[N];
    const DnxView<R> v(a, lg, ls0, ls1, lc);
    const int x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    const int y = blockIdx.y * DN_TH + threadIdx.x / DN_TW;
    const int W = (int)a.W, H = (int)a.H;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * a.W + x;
    const int step = (int)a.step;
    const float4 sp0 = v.sig0(x, y), sp1 = v.sig1(x, y);
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[i];
    // vp[h]: half h is valid at the centre.  Half h's colour distances are the other half's: they are
    // taken where the other half is valid at the centre, against den[h] from the 3x3 blur of the other
    // half's variance (clamped coordinates; an invalid pixel counts as variance 0)
    const bool vp[2] = {!(sp0.w < 0.f), !(sp1.w < 0.f)};
    float den[2] = {0.f, 0.f}, lp[2] = {0.f, 0.f};
    if (vp[0] || vp[1]) {
        float vb0 = 0.f, vb1 = 0.f;
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = min(max(y + dy, 0), H - 1);
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = min(max(x + dx, 0), W - 1);
                const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
                vb0 = vb0 + k * dn_max(v.sig0(qx, qy).w, 0.f);
                vb1 = vb1 + k * dn_max(v.sig1(qx, qy).w, 0.f);
            }
        }
        if (vp[1]) {
            den[0] = a.sigma_color * sqrtf(vb1) + 1e-6f;
            lp[0] = dn_lum(sp1);
        }
        if (vp[0]) {
            den[1] = a.sigma_color * sqrtf(vb0) + 1e-6f;
            lp[1] = dn_lum(sp0);
        }
    }
    float sw[2] = {0.f, 0.f}, sr[2] = {0.f, 0.f}, sg[2] = {0.f, 0.f}, sb[2] = {0.f, 0.f}, sv[2] = {0.f, 0.f};
    for (int iy = -2; iy <= 2; ++iy) {
        const int qy = y + iy * step;
        if (qy < 0 || qy >= H) continue;
        const float hy = iy == 0 ? 0.375f : (iy == 1 || iy == -1 ? 0.25f : 0.0625f);
        for (int ix = -2; ix <= 2; ++ix) {
            const int qx = x + ix * step;
            if (qx < 0 || qx >= W) continue;
            const float4 sq[2] = {v.sig0(qx, qy), v.sig1(qx, qy)};
            const bool vq[2] = {!(sq[0].w < 0.f), !(sq[1].w < 0.f)};
            if (!vq[0] && !vq[1]) continue;
            const float hx = ix == 0 ? 0.375f : (ix == 1 || ix == -1 ? 0.25f : 0.0625f);
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
                sw[h] = sw[h] + w;
                sr[h] = sr[h] + w * sq[h].x;
                sg[h] = sg[h] + w * sq[h].y;
                sb[h] = sb[h] + w * sq[h].z;
                sv[h] = sv[h] + (w * w) * sq[h].w;
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float4 o = make_float4(0.f, 0.f, 0.f, -1.f);
        if (sw[h] > 0.f) o = make_float4(sr[h] / sw[h], sg[h] / sw[h], sb[h] / sw[h], sv[h] / (sw[h] * sw[h]));
        a.sig_out[h][i] = o;
    }
}

// Average and remodulate: cropped pixels {((s_0 + s_1) * 0.5) * a_d, alpha, 1} and, in the error image,
// {t * t per channel, alpha, 1} with t = ((s_0 - s_1) * 0.5) * a_d; a pixel with an invalid half gets the
// beauty's mean and error 0; border pixels zero (sig_in: the last pass's output).
__global__ void __launch_bounds__(256) k_dnx_finalize(DnxArgs a) {
    const size_t n = (size_t)a.totalW * a.totalH;
    const size_t ti = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ti >= n) return;
    const uint32_t tx = (uint32_t)(ti % a.totalW), ty = (uint32_t)(ti / a.totalW);
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, e[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (tx >= a.fb && ty >= a.fb && tx - a.fb < a.W && ty - a.fb < a.H) {
        const size_t i = (size_t)(ty - a.fb) * a.W + (tx - a.fb);
        const float4 s0 = a.sig_in[0][i], s1 = a.sig_in[1][i], ce = a.centre[i];
        if (s0.w < 0.f || s1.w < 0.f) {
            float c[4];
            dn_mean(a.beauty + ti * 5, c);
            o[0] = c[0];
            o[1] = c[1];
            o[2] = c[2];
        } else {
            o[0] = ((s0.x + s1.x) * 0.5f) * ce.x;
            o[1] = ((s0.y + s1.y) * 0.5f) * ce.y;
            o[2] = ((s0.z + s1.z) * 0.5f) * ce.z;
            const float tr = ((s0.x - s1.x) * 0.5f) * ce.x;
            const float tg = ((s0.y - s1.y) * 0.5f) * ce.y;
            const float tb = ((s0.z - s1.z) * 0.5f) * ce.z;
            e[0] = tr * tr;
            e[1] = tg * tg;
            e[2] = tb * tb;
        }
        o[3] = e[3] = ce.w;
        o[4] = e[4] = 1.f;
    }
    for (int k = 0; k < 5; ++k) a.out[ti * 5 + k] = o[k];
    if (a.error)
        for (int k = 0; k < 5; ++k) a.error[ti * 5 + k] = e[k];
}

}  // namespace nd
