// The a-trous denoiser over K part images that share their guides (include/nart_hip.h, "Denoised parts":
// light groups, depth layers): for every part the bits of device/denoise.h run on that part alone.
//
// What a tap's weight takes from the guides -- w_n and d_g: the normal dot product and its squarings, the
// depth division, the coverage division -- does not depend on the part, so a launch handles a chunk of
// C parts (1..4, a template value) and computes it once per tap; per part it computes d_l, the falloff
// f(d_g + d_l), the weight and the five sums.  The arithmetic and the tile view are denoise.h's own
// (dn_guides, dn_slope, dn_signal, dn_tap_guide, dn_tap_falloff, dn_blur_variance, DnSums, dn_remodulate,
// DnTile<R, C>): nothing of them is restated here.
//   k_dnp_prepare       albedo and normal -> guide {n.xyz, z}, cov, a_d, slope, once; every part ->
//                       its signal {s.rgb, v} and alpha
//   k_dnp_variance<C>   7x7 guide-weighted luminance variance of C parts; u = w_n * f(d_g) is shared
//   k_dnp_atrous<R, C>  one 5x5 pass with holes over C parts
//   k_dnp_finalize      remodulate the parts of a chunk into their totalW x totalH nart_pixel outputs
//   k_parts_sum         ((out_0 + out_1) + out_2) + ... over the finalised images
// Launch shape and staging are denoise.h's: 32 x 8 pixel tiles, one lane per cropped pixel; the variance
// window and the passes of step 1 and 2 stage tile plus halo in LDS, 20 + 16 C bytes per staged pixel
// (at most 640 pixels: 53,760 B at C = 4); larger steps read global memory.  No atomics.
// Only the spatial variance estimate exists here: the sample-variance mode would need a second-moment
// image per part.
#pragma once

#include "denoise.h"

namespace nd {

constexpr uint32_t DNP_MAX_PARTS = 9;  // NART_DENOISE_PARTS_MAX: 8 light groups, or the 9 layers of 8 cuts
constexpr int DNP_MAX_CHUNK = 4;

struct DnpArgs : DnFilterArgs {
    // guides of all parts: nart_pixel images of totalW x totalH
    const float* albedo;
    const float* normal;
    // the parts of the launch (k_dnp_prepare: all n <= 9 of them; the others: the n <= 4 of a chunk):
    // nart_pixel images in and out, and work buffers over the cropped W x H image
    const float* part[DNP_MAX_PARTS];
    float* out[DNP_MAX_PARTS];
    const float4* sig_in[DNP_MAX_PARTS];  // {s.rgb, v}; v < 0 marks an invalid pixel (s = 0)
    float4* sig_out[DNP_MAX_PARTS];
    float* alpha[DNP_MAX_PARTS];
    // shared work buffers over the cropped image
    float4* guide;  // {n.xyz, z}; an empty pixel is all zeros (z == 0 marks it)
    float* cov;
    float4* ad;     // {a_d.rgb, 0}
    float* slope;
    uint32_t n;
};

struct PartsSumArgs {
    const float* in[DNP_MAX_PARTS];
    float* out;
    uint32_t n;
    uint64_t n_pixels;  // totalW * totalH
};

__global__ void __launch_bounds__(256) k_dnp_prepare(DnpArgs a) {
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    float4 g, ce;
    float cov;
    dn_guides(a, p.ti, g, cov, ce);
    const float slope = dn_slope(a, p.x, p.y, p.ti, g.w);
    a.guide[p.i] = g;
    a.cov[p.i] = cov;
    a.ad[p.i] = make_float4(ce.x, ce.y, ce.z, 0.f);
    a.slope[p.i] = slope;
#pragma unroll
    for (uint32_t k = 0; k < DNP_MAX_PARTS; ++k) {  // (constant indices: the arguments stay in registers)
        if (k < a.n) {
            float c[4];
            dn_mean(a.part[k] + p.ti * 5, c);
            a.sig_out[k][p.i] = dn_valid(c) ? dn_signal(c, ce, 0.f) : dn_invalid_signal();
            a.alpha[k][p.i] = c[3];
        }
    }
}

template <int C>
__global__ void __launch_bounds__(256) k_dnp_variance(DnpArgs a) {
    constexpr int R = 3;
    using Tile = DnTile<R, C, DnpArgs>;
    __shared__ typename Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y;
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    float su[C], sl[C], sl2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) su[c] = sl[c] = sl2[c] = 0.f;
    for (int dy = -R; dy <= R; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)a.H) continue;
        for (int dx = -R; dx <= R; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)a.W) continue;
            // of every part: an invalid tap is skipped per part below
            const float u = dn_window_weight(a, v, gp, covp, slope_p, dx, dy, qx, qy);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 sq = v.sig(c, qx, qy);
                if (sq.w < 0.f) continue;
                const float l = dn_lum(sq);
                su[c] = su[c] + u;
                sl[c] = sl[c] + u * l;
                sl2[c] = sl2[c] + u * (l * l);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float4 sp = v.sig(c, x, y);
        if (!(sp.w < 0.f)) {  // (an invalid pixel stays as it is)
            const float m1 = sl[c] / su[c], m2 = sl2[c] / su[c];
            sp.w = dn_max(0.f, m2 - m1 * m1);
        }
        a.sig_out[c][p.i] = sp;
    }
}

template <int R, int C>
__global__ void __launch_bounds__(256) k_dnp_atrous(DnpArgs a) {
    using Tile = DnTile<R, C, DnpArgs>;
    __shared__ typename Tile::Lds lds;
    const Tile v(a, lds);
    const DnPixel p = dn_pixel(a);
    if (!p.inside) return;
    const int x = p.x, y = p.y, W = (int)a.W, H = (int)a.H;
    const int step = (int)a.step;
    const float4 gp = v.guide(x, y);
    const float covp = v.cov(x, y), slope_p = a.slope[p.i];
    // per part: the colour distance's denominator from the blurred variance, where the centre is valid
    bool valid_p[C];
    float den[C], lp[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 sp = v.sig(c, x, y);
        valid_p[c] = !(sp.w < 0.f);
        den[c] = 0.f;
        lp[c] = 0.f;
        if (valid_p[c]) {
            den[c] = a.sigma_color * sqrtf(dn_blur_variance(v, c, x, y, W, H)) + 1e-6f;
            lp[c] = dn_lum(sp);
        }
    }
    DnSums sum[C];
    for (int iy = -2; iy <= 2; ++iy) {
        const int qy = y + iy * step;
        if (qy < 0 || qy >= H) continue;
        const float hy = dn_tap5(iy);
        for (int ix = -2; ix <= 2; ++ix) {
            const int qx = x + ix * step;
            if (qx < 0 || qx >= W) continue;
            const float hx = dn_tap5(ix);
            const bool centre = ix == 0 && iy == 0;
            float wn = 1.f, dg = 0.f;  // of every part
            if (!centre) {
                const int cheb = step * max(abs(ix), abs(iy));
                dn_tap_guide(a, gp, covp, slope_p, v.guide(qx, qy), v.cov(qx, qy), (float)cheb, wn, dg);
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 sq = v.sig(c, qx, qy);
                if (sq.w < 0.f) continue;
                float w = hx * hy;
                if (!centre) {
                    const float d_l = valid_p[c] ? dn_abs(lp[c] - dn_lum(sq)) / den[c] : 0.f;
                    w = w * dn_tap_falloff(wn, dg, d_l);
                }
                sum[c].add(w, sq);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) a.sig_out[c][p.i] = sum[c].result();
}

// Remodulate the a.n <= 4 parts of a chunk: cropped pixels {s * a_d, alpha, 1}, border pixels zero
// (sig_in: the last pass's output).
__global__ void __launch_bounds__(256) k_dnp_finalize(DnpArgs a) {
    const size_t n = (size_t)a.totalW * a.totalH;
    const size_t ti = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (ti >= n) return;
    size_t i;
    const bool inside = dn_cropped(a, ti, i);
    const float4 ce = inside ? a.ad[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < DNP_MAX_CHUNK; ++c) {
        if ((uint32_t)c < a.n) {
            float o[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (inside) dn_remodulate(a.sig_in[c][i], ce, a.alpha[c][i], o);
            dn_store_pixel(a.out[c], ti, o);
        }
    }
}

// The sum of a.n images per pixel of the total image and channel of r, g, b: it starts from image 0
// itself (no 0 is added: -0 stays) and adds the others in ascending order; alpha and filter_weight_sum
// are image 0's.
__global__ void __launch_bounds__(256) k_parts_sum(PartsSumArgs a) {
    const uint64_t ti = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (ti >= a.n_pixels) return;
    const float* p0 = a.in[0] + ti * 5;
    float o[5] = {p0[0], p0[1], p0[2], p0[3], p0[4]};
#pragma unroll
    for (uint32_t k = 1; k < DNP_MAX_PARTS; ++k) {
        if (k < a.n) {
            const float* pk = a.in[k] + ti * 5;
            o[0] = o[0] + pk[0];
            o[1] = o[1] + pk[1];
            o[2] = o[2] + pk[2];
        }
    }
    for (int k = 0; k < 5; ++k) a.out[ti * 5 + k] = o[k];
}

}  // namespace nd
