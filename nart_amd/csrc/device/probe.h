// Test hook: the device functions of dmath.h, path.h and volume.h on caller-supplied inputs
// (nart_hip_eval, include/nart_hip.h: the record layout per op is documented there).  One lane per
// record.  The probe only calls the functions the render kernels call; it holds no copy of their
// bodies, and no render path launches it.
#pragma once

#include "../../../include/nart_hip.h"
#include "volume.h"

namespace nd {

struct ProbeShade {  // the shading record (nart_hip.h)
    BxDF b;
    bool uap;
    uint32_t flags;
    float eta_outer, s1;
    f3 wo, wi;
    f2 sample;
};
ND ProbeShade probe_shade_in(const float* in, bool sampled) {
    ProbeShade p;
    const uint32_t w = __float_as_uint(in[0]);
    p.b.type = (int)(w & 0xFFu);
    p.b.flags = 0u;
    p.uap = ((w >> 8) & 1u) != 0u;
    p.flags = (w >> 16) & 0xFFu;
    p.b.rho = F3(in[1], in[2], in[3]);
    p.b.tau = F3(in[4], in[4] * 0.5f, in[4] * 0.25f);
    p.b.eta = in[5];
    p.b.a0 = in[6];
    p.b.ap = in[7];
    p.eta_outer = in[8];
    p.wo = F3(in[9], in[10], in[11]);
    p.wi = sampled ? F3(0.f, 0.f, 0.f) : F3(in[12], in[13], in[14]);
    p.s1 = sampled ? in[12] : 0.f;
    p.sample = sampled ? F2(in[13], in[14]) : F2(0.f, 0.f);
    return p;
}

// the two functions templated on the feature mask
template <uint32_t FM>
ND void probe_fm(uint32_t op, const float* in, float* out) {
    if (op == NART_EVAL_BXDF_F_PDF) {
        const ProbeShade p = probe_shade_in(in, false);
        float pdf;
        const f3 f = bxdf_f_pdf<FM>(p.b, p.wo, p.wi, p.uap, p.eta_outer, pdf);
        out[0] = f.x;
        out[1] = f.y;
        out[2] = f.z;
        out[3] = pdf;
    } else {
        const ProbeShade p = probe_shade_in(in, true);
        f3 wi = F3(0.f, 0.f, 0.f);
        float pdf = 0.f, alpha_i = -1.f;
        uint32_t flags = p.flags;
        const f3 f = bxdf_sample_f<FM>(p.b, p.wo, wi, p.s1, p.sample, pdf, flags, &alpha_i, p.uap, p.eta_outer);
        out[0] = f.x;
        out[1] = f.y;
        out[2] = f.z;
        out[3] = wi.x;
        out[4] = wi.y;
        out[5] = wi.z;
        out[6] = pdf;
        out[7] = __uint_as_float(flags);
        out[8] = alpha_i;
    }
}

// the masks nart_hip_eval accepts: the generic build and, per BxDF kind, the narrowest mask that creates it
NHD bool probe_fm_ok(uint32_t fm) {
    return fm == FT_ALL || fm == FT_LAMBERT || fm == FT_SPECMAT || fm == FT_GLASS || fm == FT_GLOSSY ||
           fm == FT_PLASTIC;
}

__global__ __launch_bounds__(256) void k_probe(uint32_t op, uint32_t fm, const float* in, uint32_t n, float* out) {
    __shared__ double2 s_logf[16];  // as k_render_volume_sm stages it
    logf_lds_stage(s_logf);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x[NART_EVAL_WORDS], y[NART_EVAL_WORDS];
#pragma unroll
    for (int k = 0; k < NART_EVAL_WORDS; ++k) {
        x[k] = in[(size_t)i * NART_EVAL_WORDS + k];
        y[k] = 0.f;
    }
    switch (op) {
        case NART_EVAL_ACOSF: y[0] = glibc_acosf(x[0]); break;
        case NART_EVAL_ATANF: y[0] = glibc_atanf(x[0]); break;
        case NART_EVAL_ATAN2F: y[0] = glibc_atan2f(x[0], x[1]); break;
        case NART_EVAL_LOGF: y[0] = glibc_logf(x[0]); break;
        case NART_EVAL_LOGF_LDS: y[0] = glibc_logf_lds(x[0], s_logf); break;
        case NART_EVAL_SINCOS:
            y[0] = glibc_sinf(x[0]);
            y[1] = glibc_cosf(x[0]);
            break;
        case NART_EVAL_F2U32: y[0] = __uint_as_float(f2u32(x[0])); break;
        case NART_EVAL_F2U8: y[0] = __uint_as_float((uint32_t)f2u8(x[0])); break;
        case NART_EVAL_GMOD: y[0] = gmod(x[0], x[1]); break;
        case NART_EVAL_GFRACT: y[0] = gfract(x[0]); break;
        case NART_EVAL_RNG_FLOAT: {
            uint32_t st = __float_as_uint(x[0]);
            y[0] = rng_float(st);
            y[1] = __uint_as_float(st);
            break;
        }
        case NART_EVAL_RNG_INT: {
            uint32_t st = __float_as_uint(x[0]);
            y[0] = __uint_as_float(rng_int(st, __float_as_uint(x[1])));
            y[1] = __uint_as_float(st);
            break;
        }
        case NART_EVAL_SAMPLE_DISK: {
            const f2 d = uniform_sample_disk(F2(x[0], x[1]));
            y[0] = d.x;
            y[1] = d.y;
            break;
        }
        case NART_EVAL_SAMPLE_RING: {
            float pdf;
            const f2 d = uniform_sample_ring(F2(x[0], x[1]), pdf, x[2]);
            y[0] = d.x;
            y[1] = d.y;
            y[2] = pdf;
            break;
        }
        case NART_EVAL_SAMPLE_COSHEMI: {
            float pdf;
            const f3 d = cosine_sample_hemisphere(F2(x[0], x[1]), pdf);
            y[0] = d.x;
            y[1] = d.y;
            y[2] = d.z;
            y[3] = pdf;
            break;
        }
        case NART_EVAL_SAMPLE_SPHERE: {
            const f3 d = uniform_sample_sphere(F2(x[0], x[1]));
            y[0] = d.x;
            y[1] = d.y;
            y[2] = d.z;
            break;
        }
        case NART_EVAL_SAMPLE_WH: {
            const f3 wh = sample_wh(F3(x[4], x[5], x[6]), x[2], F2(x[0], x[1]), __float_as_uint(x[3]) != 0u);
            y[0] = wh.x;
            y[1] = wh.y;
            y[2] = wh.z;
            break;
        }
        case NART_EVAL_FRESNEL: y[0] = fresnel(x[0], x[1], x[2]); break;
        case NART_EVAL_BXDF_F: {
            const ProbeShade p = probe_shade_in(x, false);
            const f3 f = bxdf_f(p.b, p.wo, p.wi, p.uap, p.eta_outer);
            y[0] = f.x;
            y[1] = f.y;
            y[2] = f.z;
            break;
        }
        case NART_EVAL_BXDF_PDF: {
            const ProbeShade p = probe_shade_in(x, false);
            y[0] = bxdf_pdf(p.b, p.wo, p.wi, p.uap, p.eta_outer);
            break;
        }
        default:  // NART_EVAL_BXDF_F_PDF, NART_EVAL_BXDF_SAMPLE_F (op and fm are validated on the host)
            switch (fm) {
                case FT_LAMBERT: probe_fm<FT_LAMBERT>(op, x, y); break;
                case FT_SPECMAT: probe_fm<FT_SPECMAT>(op, x, y); break;
                case FT_GLASS: probe_fm<FT_GLASS>(op, x, y); break;
                case FT_GLOSSY: probe_fm<FT_GLOSSY>(op, x, y); break;
                case FT_PLASTIC: probe_fm<FT_PLASTIC>(op, x, y); break;
                default: probe_fm<FT_ALL>(op, x, y); break;
            }
            break;
    }
#pragma unroll
    for (int k = 0; k < NART_EVAL_WORDS; ++k) out[(size_t)i * NART_EVAL_WORDS + k] = y[k];
}

}  // namespace nd
