// Test hook: the scene-bound device functions of path.h, envlight.h and volume.h -- tex_fetch,
// env_ptn_pdf, light_li / light_bound / light_sample_li, create_bsdf, dg_lookup / dg_lookup2,
// medium_sample_ray / maj_next -- on caller-supplied records against the context's device scene
// (nart_hip_scene_eval, include/nart_hip.h: the record layout per op is documented there).  One lane per
// record, 256-lane blocks.  Like probe.h and trace_probe.h it only calls the functions the render kernels
// call and holds no copy of their bodies, and no render path launches it.
#pragma once

#include "../../../include/nart_hip.h"
#include "../host/path_build.h"  // FM_DIFFUSE, FM_GLASS, FM_ENVTEX: the masks the path kernels are built for
#include "volume.h"

namespace nd {

struct SceneProbeArgs {
    const float* in = nullptr;  // n records of NART_SCENE_IN_WORDS
    float* out = nullptr;       // n records of NART_SCENE_OUT_WORDS
    uint32_t n = 0;
    uint32_t op = 0;         // NART_SCENE_*
    uint32_t build = 0;      // NART_SCENE_BUILD_*
    uint32_t lds_cells = 0;  // DG_LOOKUP: density-grid cells staged in LDS (RenderArgs::lds_nodes of the volume kernel)
};

// the (ENV, FM) pair of a NART_SCENE_BUILD_*: the builds of render.hip's table
struct SceneBuild {
    bool env;
    uint32_t fm;
};
NHD SceneBuild scene_build_of(uint32_t build) {
    switch (build) {
        case NART_SCENE_BUILD_ALL: return {false, FT_ALL};
        case NART_SCENE_BUILD_DIFFUSE: return {false, FM_DIFFUSE};
        case NART_SCENE_BUILD_GLASS: return {false, FM_GLASS};
        case NART_SCENE_BUILD_ENVTEX: return {true, FM_ENVTEX};
        default: return {true, FT_ALL};
    }
}
// plan_build's rule (host/path_build.h): the build's mask covers the scene's, a narrow mask goes with
// the scene's has_env, and an ENV = false build never meets an environment light
NHD bool scene_build_fits(uint32_t build, uint32_t features, bool has_env) {
    const SceneBuild b = scene_build_of(build);
    if ((features & ~b.fm) != 0u) return false;
    return b.fm == FT_ALL ? (b.env || !has_env) : b.env == has_env;
}

ND void scene_probe_lobe(const BxDF& b, float* y) {
    y[0] = __uint_as_float((uint32_t)b.type);
    y[1] = __uint_as_float(b.flags);
    y[2] = b.rho.x;
    y[3] = b.rho.y;
    y[4] = b.rho.z;
    y[5] = b.tau.x;
    y[6] = b.tau.y;
    y[7] = b.tau.z;
    y[8] = b.eta;
    y[9] = b.a0;
    y[10] = b.ap;
}

// the ops templated on the build
template <bool ENV, uint32_t FM>
ND void scene_probe_fm(const DScene& S, uint32_t op, const float* x, float* y) {
    if (op == NART_SCENE_CREATE_BSDF) {
        Isect is;
        is.p = is.gn = is.dpdt = F3(0.f, 0.f, 0.f);
        is.meshID = is.priority = 0u;
        is.mat = __float_as_uint(x[0]);
        is.st = F2(x[1], x[2]);
        is.sn = F3(x[3], x[4], x[5]);
        is.dpds = F3(x[6], x[7], x[8]);
        BSDF bs;
        bs.n = bs.n_t = bs.n_b = F3(0.f, 0.f, 0.f);
        bs.num = 0u;
        for (int k = 0; k < 2; ++k) {
            bs.b[k].type = 0;
            bs.b[k].flags = 0u;
            bs.b[k].rho = bs.b[k].tau = F3(0.f, 0.f, 0.f);
            bs.b[k].eta = bs.b[k].a0 = bs.b[k].ap = 0.f;
        }
        create_bsdf<FM>(S, is, x[9], bs);
        y[0] = bs.n.x;
        y[1] = bs.n.y;
        y[2] = bs.n.z;
        y[3] = bs.n_t.x;
        y[4] = bs.n_t.y;
        y[5] = bs.n_t.z;
        y[6] = bs.n_b.x;
        y[7] = bs.n_b.y;
        y[8] = bs.n_b.z;
        y[9] = __uint_as_float(bs.num);
        scene_probe_lobe(bs.b[0], y + 10);
        if (bs.num > 1u) scene_probe_lobe(bs.b[1], y + 21);
        return;
    }
    const DLight& L = uniform_light(S, __float_as_uint(x[0]));
    const f3 p = F3(x[1], x[2], x[3]);
    float pdf = x[9], tMax = x[10];
    if (op == NART_SCENE_LIGHT_LI) {
        const f3 Li = light_li<ENV, FM>(S, L, p, F3(x[4], x[5], x[6]), __float_as_uint(x[7]) ? &pdf : nullptr, tMax, x[8]);
        y[0] = Li.x;
        y[1] = Li.y;
        y[2] = Li.z;
        y[3] = pdf;
        y[4] = tMax;
    } else if (op == NART_SCENE_LIGHT_BOUND) {
        light_bound<ENV, FM>(L, p, F3(x[4], x[5], x[6]), tMax);
        y[4] = tMax;
    } else {  // NART_SCENE_LIGHT_SAMPLE_LI
        f3 wi = F3(0.f, 0.f, 0.f);
        const f3 Li = light_sample_li<ENV, FM>(S, L, p, wi, F2(x[4], x[5]), pdf, tMax);
        y[0] = Li.x;
        y[1] = Li.y;
        y[2] = Li.z;
        y[3] = pdf;
        y[4] = tMax;
        y[5] = wi.x;
        y[6] = wi.y;
        y[7] = wi.z;
    }
}

// op, build and every record's indices are validated on the host (nart_hip_scene_eval)
__global__ __launch_bounds__(256) void k_scene_probe(DScene S, SceneProbeArgs P) {
    extern __shared__ float s_dens[];  // as k_render_volume_sm stages the density grid
    if (P.op == NART_SCENE_DG_LOOKUP && P.lds_cells) dens_lds_stage(s_dens, S.medium.density, P.lds_cells);
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    float x[NART_SCENE_IN_WORDS], y[NART_SCENE_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < NART_SCENE_IN_WORDS; ++k) x[k] = P.in[(size_t)i * NART_SCENE_IN_WORDS + k];
#pragma unroll
    for (int k = 0; k < NART_SCENE_OUT_WORDS; ++k) y[k] = 0.f;
    const DMedium& m = S.medium;
    switch (P.op) {
        case NART_SCENE_TEX_FETCH: {
            const f3 c = tex_fetch(S, (int)__float_as_uint(x[0]), x[1], x[2], (int)__float_as_uint(x[3]));
            y[0] = c.x;
            y[1] = c.y;
            y[2] = c.z;
            break;
        }
        case NART_SCENE_ENV_PDF: y[0] = env_ptn_pdf(S, uniform_light(S, __float_as_uint(x[0])), F2(x[1], x[2])); break;
        case NART_SCENE_DG_LOOKUP: {
            const f3 p = F3(x[0], x[1], x[2]);
            y[0] = dg_lookup(m, m.density, p);
            y[1] = dg_lookup(m, P.lds_cells ? s_dens : m.density, p);
            if (m.grid2) {
                y[2] = dg_lookup2(m, p);
                y[3] = __uint_as_float(1u);
            }
            break;
        }
        case NART_SCENE_MEDIUM_WALK: {
            MajIter it;
            it.tCurrent = it.tMax = 0.f;
            const bool ok = medium_sample_ray(m, F3(x[0], x[1], x[2]), F3(x[3], x[4], x[5]), it);
            y[0] = __uint_as_float(ok ? 1u : 0u);
            uint32_t ns = 0;
            if (ok) {
                y[2] = it.tCurrent;
                y[3] = it.tMax;
                float sigma, t0, t1;
                uint32_t used = 0;
#pragma unroll
                for (int k = 0; k < NART_SCENE_WALK_SEGMENTS; ++k) {
                    if (ns == (uint32_t)k && maj_next(m, it, sigma, t0, t1, &used)) {
                        y[4 + 4 * k] = sigma;
                        y[5 + 4 * k] = t0;
                        y[6 + 4 * k] = t1;
                        y[7 + 4 * k] = __uint_as_float(used);
                        ++ns;
                    }
                }
            }
            y[1] = __uint_as_float(ns);
            break;
        }
        default:  // the light ops and CREATE_BSDF
            switch (P.build) {
                case NART_SCENE_BUILD_ALL: scene_probe_fm<false, FT_ALL>(S, P.op, x, y); break;
                case NART_SCENE_BUILD_DIFFUSE: scene_probe_fm<false, FM_DIFFUSE>(S, P.op, x, y); break;
                case NART_SCENE_BUILD_GLASS: scene_probe_fm<false, FM_GLASS>(S, P.op, x, y); break;
                case NART_SCENE_BUILD_ENVTEX: scene_probe_fm<true, FM_ENVTEX>(S, P.op, x, y); break;
                default: scene_probe_fm<true, FT_ALL>(S, P.op, x, y); break;
            }
            break;
    }
#pragma unroll
    for (int k = 0; k < NART_SCENE_OUT_WORDS; ++k) P.out[(size_t)i * NART_SCENE_OUT_WORDS + k] = y[k];
}

}  // namespace nd
