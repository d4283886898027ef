// Edge-avoiding a-trous denoiser over the first-hit AOVs (include/nart_hip.h, nart_hip_denoise).
//
// Four kernels, one lane per cropped-image pixel, lanes along x, 32 x 8 pixel tiles (256 threads),
// no atomics: every output is a pure function of its inputs, whatever the launch shape.
//   k_dn_prepare   the three nart_pixel images -> guide {n.xyz, z}, cov, signal {s.rgb, v},
//                  centre record {a_d.rgb, alpha} and depth slope
//   k_dn_variance  7x7 guide-weighted luminance variance into signal.v
//                  (not launched in the sample-variance mode: k_dn_prepare<true> writes signal.v
//                  from the renderer's second-moment image, see below)
//   k_dn_atrous    one 5x5 pass with holes (step 2^i), signal ping-pong
//   k_dn_finalize  remodulate into the totalW x totalH nart_pixel output
// The variance window and the passes of step 1 and 2 stage their tile plus halo in LDS (R = 3, 2, 4
// pixels of halo: 36 B per staged pixel, at most 40 x 16 pixels = 22.5 KB); larger steps read global
// memory (R = 0), where the 36 B per tap come out of the cache hierarchy.  Both ways run the same
// arithmetic in the same order.  Which kernel runs when, with which halo and between which signal
// buffers, is host/denoise_passes.h's plan.
//
// What the cross-filtered and the parts denoiser (denoise_cross.h, denoise_parts.h) share with this one is
// defined here once, each piece stating the operation order it fixes: the tile view DnTile<R, S, Args>
// over S signals, the lane's pixel (dn_pixel, dn_cropped), the guide arithmetic (dn_guides, dn_slope,
// dn_tap_guide, dn_tap_falloff, dn_window_weight), the 5-tap weight (dn_tap5), the 3x3 variance blur
// (dn_blur_variance), the sums of a pass (DnSums) and the remodulation (dn_remodulate).
//
// The arithmetic is float32 + - * / sqrt and comparisons only, in the order the header fixes, built
// without contraction: tests/denoise_py.py restates it in numpy and the images agree bit for bit.
// min and max are written as comparisons (dn_min, dn_max) so that their NaN and signed-zero
// behaviour is the restatement's np.where, not a library's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nd {

// What the three denoisers' argument structs (DnArgs, DnxArgs of denoise_cross.h, DnpArgs of
// denoise_parts.h) share: the image layout, the step of the launch and nart_denoise_params' filter fields.
struct DnFilterArgs {
    uint32_t W, H, totalW, totalH, fb;
    uint32_t step;
    uint32_t normal_squarings;
    float sigma_color, sigma_depth, depth_eps, sigma_coverage, albedo_floor;
};

struct DnArgs : DnFilterArgs {
    // inputs / output: nart_pixel images of totalW x totalH, 5 floats per pixel
    const float* beauty;
    const float* albedo;
    const float* normal;
    const float* moment;  // second-moment image (k_dn_prepare<true> only), else null
    float* out;
    // work buffers over the cropped W x H image
    float4* guide;       // {n.xyz, z}; an empty pixel is all zeros (z == 0 marks it)
    float* cov;
    const float4* sig_in[1];  // {s.rgb, v}; v < 0 marks an invalid pixel (s = 0)
    float4* sig_out[1];
    float4* centre;      // {a_d.rgb, alpha}
    float* slope;
};

constexpr int DN_TW = 32, DN_TH = 8;  // pixels per block: 256 lanes, lanes along x

__device__ __forceinline__ float dn_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float dn_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float dn_abs(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ bool dn_finite(float a) { return dn_abs(a) < __builtin_inff(); }
__device__ __forceinline__ float dn_lum(const float4& s) { return (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z; }

// Mean depth over hit samples of total-image pixel ti: normal.w / albedo.a, 0 for an empty pixel.
// (Args: DnArgs, or the parts' DnpArgs of denoise_parts.h, which names the same fields.)
template <class Args>
__device__ __forceinline__ float dn_depth(const Args& a, size_t ti) {
    const float hs = a.albedo[ti * 5 + 3];
    return hs > 0.f ? a.normal[ti * 5 + 3] / hs : 0.f;
}

// c = P.rgba / P.w of a nart_pixel, 0 if P.w <= 0.
__device__ __forceinline__ void dn_mean(const float* P, float c[4]) {
    c[0] = c[1] = c[2] = c[3] = 0.f;
    if (P[4] > 0.f)
        for (int k = 0; k < 4; ++k) c[k] = P[k] / P[4];
}

// What prepare takes from the albedo and normal images alone, for cropped pixel (x, y) = total-image
// pixel ti: the guide g = {n.xyz, z}, cov, the demodulation albedo ce.xyz = a_d (ce.w is left alone)
// (dn_guides), and the depth slope around a pixel of depth z (dn_slope).
template <class Args>
__device__ __forceinline__ void dn_guides(const Args& a, size_t ti, float4& g, float& cov, float4& ce) {
    const float* A = a.albedo + ti * 5;
    const float* N = a.normal + ti * 5;
    float al[3] = {0.f, 0.f, 0.f};
    cov = 0.f;
    if (A[4] > 0.f) {
        for (int k = 0; k < 3; ++k) al[k] = A[k] / A[4];
        cov = A[3] / A[4];
    }
    const float hs = A[3];
    g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (hs > 0.f) {
        g.w = N[3] / hs;
        if (g.w != 0.f) {
            g.x = N[0] / hs;
            g.y = N[1] / hs;
            g.z = N[2] / hs;
        } else {
            g.w = 0.f;  // -0 -> +0
        }
    }
    const float miss = 1.f - cov;
    ce.x = dn_max(al[0] + miss, a.albedo_floor);
    ce.y = dn_max(al[1] + miss, a.albedo_floor);
    ce.z = dn_max(al[2] + miss, a.albedo_floor);
}

// Depth slope: per axis the smaller one-sided |dz| (the one available at a border, 0 on a
// single-pixel axis).
template <class Args>
__device__ __forceinline__ float dn_slope(const Args& a, uint32_t x, uint32_t y, size_t ti, float z) {
    float sx = 0.f, sy = 0.f;
    if (a.W > 1) {
        const float dl = x > 0 ? dn_abs(z - dn_depth(a, ti - 1)) : 0.f;
        const float dr = x + 1 < a.W ? dn_abs(dn_depth(a, ti + 1) - z) : 0.f;
        sx = x == 0 ? dr : (x + 1 == a.W ? dl : dn_min(dl, dr));
    }
    if (a.H > 1) {
        const float du = y > 0 ? dn_abs(z - dn_depth(a, ti - a.totalW)) : 0.f;
        const float dd = y + 1 < a.H ? dn_abs(dn_depth(a, ti + a.totalW) - z) : 0.f;
        sy = y == 0 ? dd : (y + 1 == a.H ? du : dn_min(du, dd));
    }
    return sx + sy;
}

// A pixel whose c.rgb has a non-finite component is invalid: signal {0, 0, 0, -1}; a valid one's is
// {c.rgb / a_d, v}.
__device__ __forceinline__ bool dn_valid(const float c[4]) { return dn_finite(c[0]) && dn_finite(c[1]) && dn_finite(c[2]); }
__device__ __forceinline__ float4 dn_invalid_signal() { return make_float4(0.f, 0.f, 0.f, -1.f); }
__device__ __forceinline__ float4 dn_signal(const float c[4], const float4& ad, float v) {
    return make_float4(c[0] / ad.x, c[1] / ad.y, c[2] / ad.z, v);
}

// Sample variance of the demodulated luminance from the second-moment pixel M (include/nart_hip.h,
// "Sample variance"): c the filtered beauty, ad the demodulation albedo.  k = sum w^2 / (sum w)^2 is
// 1 / the effective sample count; per channel the weighted second moment minus the squared mean,
// clamped at 0, times k is the variance of the filtered mean.  No Bessel correction is applied (the
// estimate is the biased one, low by the factor 1 - k).  The channel standard deviations are summed
// with the luminance weights, i.e. the channels' noise counts as fully correlated: the conservative
// bound, and what one light path hitting or missing produces.  NaN and overflow become 1e30.
__device__ __forceinline__ float dn_sample_variance(const float* M, const float* c, const float4& ad) {
    float V[3] = {0.f, 0.f, 0.f};
    const float mw = M[4];
    if (mw > 0.f) {
        const float k = M[3] / (mw * mw);
        for (int ch = 0; ch < 3; ++ch) {
            const float m2 = M[ch] / mw;
            const float var = dn_max(0.f, m2 - c[ch] * c[ch]);
            V[ch] = var * k;
        }
    }
    const float sd = (0.2126f * (sqrtf(V[0]) / ad.x) + 0.7152f * (sqrtf(V[1]) / ad.y)) + 0.0722f * (sqrtf(V[2]) / ad.z);
    const float v = sd * sd;
    return v < 1e30f ? v : 1e30f;
}

// The pixel of a lane of the 32 x 8 tile kernels: cropped coordinates (lanes along x), the pixel's index i
// in the work buffers and ti in the total image; inside: the lane has a pixel.
struct DnPixel {
    int x, y;
    size_t i, ti;
    bool inside;
};
template <class Args>
__device__ __forceinline__ DnPixel dn_pixel(const Args& a) {
    DnPixel p;
    p.x = blockIdx.x * DN_TW + (threadIdx.x & (DN_TW - 1));
    p.y = blockIdx.y * DN_TH + threadIdx.x / DN_TW;
    p.inside = p.x < (int)a.W && p.y < (int)a.H;
    p.i = (size_t)p.y * a.W + p.x;
    p.ti = (size_t)(p.y + a.fb) * a.totalW + (p.x + a.fb);
    return p;
}

// The pixel of a lane of the finalize kernels, one lane per total-image pixel ti (the caller has checked
// ti < totalW * totalH): whether it lies in the cropped window, and then its index i there.
template <class Args>
__device__ __forceinline__ bool dn_cropped(const Args& a, size_t ti, size_t& i) {
    const uint32_t tx = (uint32_t)(ti % a.totalW), ty = (uint32_t)(ti / a.totalW);
    const bool inside = tx >= a.fb && ty >= a.fb && tx - a.fb < a.W && ty - a.fb < a.H;
    i = inside ? (size_t)(ty - a.fb) * a.W + (tx - a.fb) : 0;
    return inside;
}

// Remodulate one pixel: {s.rgb * a_d.rgb, alpha, 1}, each channel one multiplication.
__device__ __forceinline__ void dn_remodulate(const float4& s, const float4& ad, float alpha, float o[5]) {
    o[0] = s.x * ad.x;
    o[1] = s.y * ad.y;
    o[2] = s.z * ad.z;
    o[3] = alpha;
    o[4] = 1.f;
}
__device__ __forceinline__ void dn_store_pixel(float* img, size_t ti, const float o[5]) {
    for (int k = 0; k < 5; ++k) img[ti * 5 + k] = o[k];
}

// MOMENT: the sample-variance mode -- everything the spatial mode's prepare computes, and signal.v
// from the moment image instead of 0 (k_dn_variance then does not run).
template <bool MOMENT>
__global__ void __launch_bounds__(256) k_dn_prepare(DnArgs a) {
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    float c[4];
    dn_mean(a.beauty + p.ti * 5, c);
    float4 g, ce;
    float cov;
    dn_guides(a, p.ti, g, cov, ce);
    ce.w = c[3];
    const bool valid = dn_valid(c);
    float4 s = dn_invalid_signal();
    if (valid) s = dn_signal(c, ce, MOMENT ? dn_sample_variance(a.moment + p.ti * 5, c, ce) : 0.f);
    const float slope = dn_slope(a, p.x, p.y, p.ti, g.w);
    a.guide[p.i] = g;
    a.cov[p.i] = cov;
    a.sig_out[0][p.i] = s;
    a.centre[p.i] = ce;
    a.slope[p.i] = slope;
}

// A block's view of the per-tap records of S signals (1: denoise.h; 2 halves: denoise_cross.h; the C
// parts of a chunk: denoise_parts.h): its tile plus R pixels of halo in LDS (R > 0), 20 + 16 S bytes per
// staged pixel, or global memory (R == 0).  A staged pixel outside the image is empty and invalid.  The
// accessors are only called with coordinates inside the image.
template <int R, int S, class Args>
struct DnTile {
    static constexpr int LW = DN_TW + 2 * R, LH = DN_TH + 2 * R;
    static constexpr int N = R > 0 ? LW * LH : 1;
    struct Lds {
        float4 g[N];
        float4 s[S * N];
        float c[N];
    };
    Lds& l;
    const Args& a;
    int x0, y0;  // image coordinates of the staged region's first pixel

    __device__ DnTile(const Args& args, Lds& lds) : l(lds), a(args) {
        x0 = (int)(blockIdx.x * DN_TW) - R;
        y0 = (int)(blockIdx.y * DN_TH) - R;
        if (R > 0) {
            for (int k = threadIdx.x; k < LW * LH; k += 256) {
                const int gx = x0 + k % LW, gy = y0 + k / LW;
                float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f), s4[S];
                float c1 = 0.f;
#pragma unroll
                for (int c = 0; c < S; ++c) s4[c] = dn_invalid_signal();
                if (gx >= 0 && gy >= 0 && gx < (int)a.W && gy < (int)a.H) {
                    const size_t i = (size_t)gy * a.W + gx;
                    g4 = a.guide[i];
#pragma unroll
                    for (int c = 0; c < S; ++c) s4[c] = a.sig_in[c][i];
                    c1 = a.cov[i];
                }
                l.g[k] = g4;
#pragma unroll
                for (int c = 0; c < S; ++c) l.s[c * N + k] = s4[c];
                l.c[k] = c1;
            }
            __syncthreads();
        }
    }
    __device__ __forceinline__ size_t idx(int x, int y) const {
        return R > 0 ? (size_t)((y - y0) * LW + (x - x0)) : (size_t)y * a.W + x;
    }
    __device__ __forceinline__ float4 guide(int x, int y) const { return R > 0 ? l.g[idx(x, y)] : a.guide[idx(x, y)]; }
    __device__ __forceinline__ float cov(int x, int y) const { return R > 0 ? l.c[idx(x, y)] : a.cov[idx(x, y)]; }
    // c is a constant after unrolling
    __device__ __forceinline__ float4 sig(int c, int x, int y) const {
        return R > 0 ? l.s[c * N + idx(x, y)] : a.sig_in[c][idx(x, y)];
    }
};

// The weight of a tap that is not the centre (include/nart_hip.h, "Guide terms"), in two halves.
// The guide half: w_n and d_g, which the guides alone decide (the same for every image filtered with
// them: denoise_parts.h and denoise_cross.h compute them once per tap for several).
template <class Args>
__device__ __forceinline__ void dn_tap_guide(const Args& a, const float4& gp, float covp, float slope_p, const float4& gq,
                                             float covq, float cheb, float& wn, float& dg) {
    wn = 1.f;
    if (!(gp.w == 0.f && gq.w == 0.f)) {
        const float dot = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
        wn = dn_min(1.f, dn_max(0.f, dot));
        for (uint32_t k = 0; k < a.normal_squarings; ++k) wn = wn * wn;
    }
    const float dz = dn_abs(gp.w - gq.w) / ((a.sigma_depth * (slope_p * cheb) + a.depth_eps * dn_max(gp.w, gq.w)) + 1e-30f);
    dg = dz + dn_abs(covp - covq) / a.sigma_coverage;
}

// The falloff half: w_n * f(d_g + d_l).
__device__ __forceinline__ float dn_tap_falloff(float wn, float dg, float d_l) {
    const float t = dn_max(0.f, 1.f - (dg + d_l) * 0.125f);
    const float t2 = t * t, t4 = t2 * t2;
    return wn * (t4 * t4);
}

// The guide-only weight u of the variance window's tap (dx, dy) of the tile, the centre's 1: both halves
// with d_l = 0 and the Chebyshev distance of the offset.
template <class Tile, class Args>
__device__ __forceinline__ float dn_window_weight(const Args& a, const Tile& v, const float4& gp, float covp, float slope_p,
                                                  int dx, int dy, int qx, int qy) {
    if (dx == 0 && dy == 0) return 1.f;
    float wn, dg;
    dn_tap_guide(a, gp, covp, slope_p, v.guide(qx, qy), v.cov(qx, qy), (float)max(abs(dx), abs(dy)), wn, dg);
    return dn_tap_falloff(wn, dg, 0.f);
}

// The B-spline weight of the tap at offset o in -2..2 along one axis: 3/8, 1/4, 1/16.
__device__ __forceinline__ float dn_tap5(int o) { return o == 0 ? 0.375f : (o == 1 || o == -1 ? 0.25f : 0.0625f); }

// 3x3 blur of signal c's variance around (x, y): weights (1/4, 1/2, 1/4) per axis, coordinates clamped
// to the image, an invalid pixel counting as variance 0; summed from 0 row by row, dy outer, dx inner.
template <class Tile>
__device__ __forceinline__ float dn_blur_variance(const Tile& v, int c, int x, int y, int W, int H) {
    float vb = 0.f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = min(max(y + dy, 0), H - 1);
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = min(max(x + dx, 0), W - 1);
            const float k = (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f);
            vb = vb + k * dn_max(v.sig(c, qx, qy).w, 0.f);
        }
    }
    return vb;
}

// The five sums of one signal's a-trous pass, from 0 in tap order: add() takes a valid tap of weight w,
// result() normalises -- {sum w s / sum w, sum w^2 v / (sum w)^2}, invalid where no weight came in.
struct DnSums {
    float w = 0.f, r = 0.f, g = 0.f, b = 0.f, v = 0.f;
    __device__ __forceinline__ void add(float wq, const float4& sq) {
        w = w + wq;
        r = r + wq * sq.x;
        g = g + wq * sq.y;
        b = b + wq * sq.z;
        v = v + (wq * wq) * sq.w;
    }
    __device__ __forceinline__ float4 result() const {
        return w > 0.f ? make_float4(r / w, g / w, b / w, v / (w * w)) : dn_invalid_signal();
    }
};

__global__ void __launch_bounds__(256) k_dn_variance(DnArgs a) {
    constexpr int R = 3;
    using Tile = DnTile<R, 1, DnArgs>;
    __shared__ Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y;
    float4 sp = v.sig(0, x, y);
    if (sp.w < 0.f) {  // invalid: stays as it is
        a.sig_out[0][p.i] = sp;
        return;
    }
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    float su = 0.f, sl = 0.f, sl2 = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)a.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)a.W) continue;
            const float4 sq = v.sig(0, qx, qy);
            if (sq.w < 0.f) continue;
            const float u = dn_window_weight(a, v, gp, covp, slope_p, dx, dy, qx, qy);
            const float l = dn_lum(sq);
            su = su + u;
            sl = sl + u * l;
            sl2 = sl2 + u * (l * l);
        }
    }
    const float m1 = sl / su, m2 = sl2 / su;
    sp.w = dn_max(0.f, m2 - m1 * m1);
    a.sig_out[0][p.i] = sp;
}

template <int R>
__global__ void __launch_bounds__(256) k_dn_atrous(DnArgs a) {
    using Tile = DnTile<R, 1, DnArgs>;
    __shared__ typename Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y, W = (int)a.W, H = (int)a.H;
    const int step = (int)a.step;
    const float4 sp = v.sig(0, x, y);
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    const bool valid_p = !(sp.w < 0.f);
    float den = 0.f, lp = 0.f;
    if (valid_p) {
        den = a.sigma_color * sqrtf(dn_blur_variance(v, 0, x, y, W, H)) + 1e-6f;
        lp = dn_lum(sp);
    }
    DnSums sum;
    for (int iy = -2; iy <= 2; ++iy) {
        const int qy = y + iy * step;
        if (qy < 0 || qy >= H) continue;
        const float hy = dn_tap5(iy);
        for (int ix = -2; ix <= 2; ++ix) {
            const int qx = x + ix * step;
            if (qx < 0 || qx >= W) continue;
            const float4 sq = v.sig(0, qx, qy);
            if (sq.w < 0.f) continue;
            float w = dn_tap5(ix) * hy;
            if (ix != 0 || iy != 0) {
                const float d_l = valid_p ? dn_abs(lp - dn_lum(sq)) / den : 0.f;
                const int cheb = step * max(abs(ix), abs(iy));
                float wn, dg;
                dn_tap_guide(a, gp, covp, slope_p, v.guide(qx, qy), v.cov(qx, qy), (float)cheb, wn, dg);
                w = w * dn_tap_falloff(wn, dg, d_l);
            }
            sum.add(w, sq);
        }
    }
    a.sig_out[0][p.i] = sum.result();
}

// Remodulate: cropped pixels {s * a_d, alpha, 1}, border pixels zero (sig_in: the last pass's output).
__global__ void __launch_bounds__(256) k_dn_finalize(DnArgs a) {
    const size_t n = (size_t)a.totalW * a.totalH;
    const size_t ti = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ti >= n) return;
    size_t i;
    float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (dn_cropped(a, ti, i)) {
        const float4 ce = a.centre[i];
        dn_remodulate(a.sig_in[0][i], ce, ce.w, o);
    }
    dn_store_pixel(a.out, ti, o);
}

}  // namespace nd
