// Followed guides (include/nart_hip.h, "Followed guides"): the denoiser guide
// records of the first non-delta surface of every camera sample.  The chain is k_render's loop
// (pathintegrator.cpp:166-258) without EstimateDirect and Russian roulette, its three continuation
// random numbers replaced by (s1, sample) = (0, (1, 0)) so that Fresnel reflection is never chosen
// (sample.x = 1 is never < Fr), and alphaTweak fixed at 1: a perfect mirror reflects, a smooth
// dielectric refracts or reflects on total internal reflection, a lower-priority interface is
// stepped through, and the first hit that is neither -- or the one reached after max_follow such
// steps -- is the guide hit.  No RNG draw, no atomics.
//   albedo record  {albedo.rgb, 1}: aov_record<AOV_ALBEDO>'s pattern choice at the guide hit
//   normal record  {normalize(bs.n).xyz, D}: D = ((t0 + t1) + t2) + ..., the float32 sum of every
//                  segment's plane distance computed as aov_record computes the first-hit depth
// A miss (no hit within the nearest analytic light on any segment) is all zeros in both.
//
// k_guide: lane = traced pixel, looping over its samples with k_aov's two access patterns; per-lane
// traversal (path.h traverse) on the [depth][lane] LDS stack of 8-B entries, 256 lanes a block,
// stack_depth * 256 * 8 bytes of LDS (k_primary's per-lane form).  The chain is bounded by
// max_follow <= GUIDE_MAX_FOLLOW and nothing else: at most 11 traversals a sample, and the
// dielectric list never outgrows its ILIST_REG registers (one update per followed segment).
// DUMP (the per-sample debug entry point only, never the frame path): every segment's ray, bound,
// plane distance and triangle.
#pragma once

#include "kernels.h"

namespace nd {

constexpr uint32_t GUIDE_MAX_FOLLOW = 10;
static_assert(GUIDE_MAX_FOLLOW <= ILIST_REG, "one list entry per followed interface, all in registers");

struct GuideArgs {
    float4* albedo = nullptr;  // per-sample records, indexed like the samples; null: not wanted
    float4* normal = nullptr;
    uint32_t max_follow = 0;
    // DUMP: [sample][max_follow + 1] segments {o.xyz, tmax, d.xyz, t} and triangles, [sample] counts
    float* seg8 = nullptr;
    uint32_t* tri = nullptr;
    uint32_t* n_seg = nullptr;
};

template <bool ENV, bool DUMP>
ND void guide_chain(const DScene& S, const RenderArgs& A, const GuideArgs& G, uint32_t px, uint32_t py, float2 sm,
                    uint64_t idx, int* sc) {
    Ray ray = cast_ray(S, F2(sm.x, sm.y), A.W, A.H, px, py);
    IList<false> list;
    list.n = 0;
    float D = 0.f;
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), rn = ra;
    TraceCounters cnt = {0u, 0u, 0u, 0u};
    const uint32_t mf = G.max_follow < GUIDE_MAX_FOLLOW ? G.max_follow : GUIDE_MAX_FOLLOW;
    uint32_t nseg = 0;
#pragma unroll 1
    for (uint32_t k = 0; k <= mf; ++k) {
        // light loop bound (pathintegrator.cpp:167-182)
        float tmax = __builtin_inff();
        for (uint32_t j = 0; j < S.num_lights; ++j) {
            float lt = __builtin_inff();
            light_bound<ENV>(uniform_light(S, j), ray.o, ray.d, lt);
            if (lt < tmax) tmax = lt;
        }
        float bt;
        uint32_t g;
        traverse<false>(S, ray, tmax, false, bt, g, sc, nullptr, (int)blockDim.x, cnt, nullptr, 0);
        float t = tmax;
        Isect is;
        if (g != NO_HIT) {
            fill_isect(S, ray, g, is);
            const nart_triangle& T = S.tris[g];
            const f3 v0 = load3(T.v0);
            const f3 pn = cross(sub(load3(T.v1), v0), sub(load3(T.v2), v0));
            t = (dot(v0, pn) - dot(ray.o, pn)) / dot(ray.d, pn);
        }
        if (DUMP) {
            const uint64_t e = idx * (uint64_t)(G.max_follow + 1u) + k;
            float4* q = reinterpret_cast<float4*>(G.seg8 + e * 8u);
            q[0] = make_float4(ray.o.x, ray.o.y, ray.o.z, tmax);
            q[1] = make_float4(ray.d.x, ray.d.y, ray.d.z, t);
            G.tri[e] = g;
            nseg = (k == 0u && g == NO_HIT) ? 0u : k + 1u;  // a camera-ray miss counts no segment
        }
        if (g == NO_HIT) break;  // a miss: both records stay zero
        BSDF bs;
        create_bsdf<FT_ALL>(S, is, 1.f, bs);
        D = D + t;
        float eta_outer = 1.f;
        const bool valid = list.valid(is.meshID, is.priority, eta_outer, nullptr, 0);
        bool follow = false;
        if (k < mf) {
            if (!valid) {
                // lower-priority interface: step through (pathintegrator.cpp:223-229)
                ray = make_ray(add(is.p, muls(ray.d, SHADOW_BIAS)), ray.d);
                list.update(is.meshID, is.priority, bsdf_sample_eta(bs, 0.f), nullptr, 0);
                follow = true;
            } else if (bs.num == 1u && (bs.b[0].type == B_SPECULAR || bs.b[0].type == B_SPECDIEL)) {
                // the continuation (pathintegrator.cpp:199-220) with (s1, sample) = (0, (1, 0))
                const f3 wo = to_local(bs, neg(ray.d));
                float pdf = 0.f, eta_sampled = 1.f;
                uint32_t flags = 0;
                f3 wi;
                bsdf_sample_f<false>(bs, wo, wi, 0.f, F2(1.f, 0.f), pdf, flags, false, eta_outer, nullptr, &eta_sampled);
                // An index-matched interface (pdf 0, no specular flag) ends the path and the chain.
                // Total internal reflection leaves the refraction branch with pdf = 1 - Fr = 0 as
                // well, but the path never gets there: its sample.x < 1 = Fr takes the reflection
                // branch, with this same wi.  So the flag decides, not pdf.
                if (flags & F_SPECULAR) {
                    const float flip = wi.z > 0.f ? 1.f : -1.f;
                    ray = make_ray(add(is.p, muls(muls(is.gn, SHADOW_BIAS), flip)), to_world(bs, wi));
                    if (flags & F_TRANSMISSIVE) list.update(is.meshID, is.priority, eta_sampled, nullptr, 0);
                    follow = true;
                }
            }
        }
        if (follow) continue;
        // the guide hit
        const DMaterial& m = cst(S.mats)[is.mat];
        const int32_t mt = m.type;
        const DPattern& p = (mt == NART_MAT_SPECULAR || mt == NART_MAT_GLOSSY) ? m.rho_s : (mt == NART_MAT_GLASS ? m.tau : m.rho_d);
        const f3 a = ptn_value<FT_ALL>(S, p, is.st);
        const f3 n = normalize(bs.n);
        ra = make_float4(a.x, a.y, a.z, 1.f);
        rn = make_float4(n.x, n.y, n.z, D);
        break;
    }
    if (G.albedo) G.albedo[idx] = ra;
    if (G.normal) G.normal[idx] = rn;
    if (DUMP) {
        G.n_seg[idx] = nseg;
        for (uint32_t k = nseg ? nseg : 1u; k <= G.max_follow; ++k) {  // never traced
            const uint64_t e = idx * (uint64_t)(G.max_follow + 1u) + k;
            float4* q = reinterpret_cast<float4*>(G.seg8 + e * 8u);
            q[0] = q[1] = make_float4(0.f, 0.f, 0.f, 0.f);
            G.tri[e] = NO_HIT;
        }
    }
}

template <bool ENV, bool DUMP>
__global__ __launch_bounds__(256) void k_guide(DScene S, RenderArgs A, GuideArgs G) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= A.n_slots) return;
    int* sc = reinterpret_cast<int*>(reinterpret_cast<int2*>(s_dyn) + threadIdx.x);  // [depth][lane] int2
    const uint32_t xy = A.slot_xy[slot];
    const uint32_t px = xy & 0xFFFFu, py = xy >> 16;
    const SlotSO so = A.slot_so[slot];
    if (so.stride == 1u && (A.spp & 7u) == 0u && (so.first & 7u) == 0u) {
        // pixel-major rows: 8 samples (64 B) per read, as k_aov
        const float4* sp = reinterpret_cast<const float4*>(A.samples + so.first);
        for (uint32_t c = 0; c < A.spp / 8u; ++c) {
            const float4 q0 = sp[4 * c], q1 = sp[4 * c + 1], q2 = sp[4 * c + 2], q3 = sp[4 * c + 3];
#pragma unroll 1
            for (uint32_t k = 0; k < 8u; ++k) {  // one call site for the eight samples
                const float4 q = k < 2u ? q0 : (k < 4u ? q1 : (k < 6u ? q2 : q3));
                guide_chain<ENV, DUMP>(S, A, G, px, py, (k & 1u) ? make_float2(q.z, q.w) : make_float2(q.x, q.y),
                                       so.first + 8u * c + k, sc);
            }
        }
    } else {
        for (uint32_t s = 0; s < A.spp; ++s) {
            const uint64_t idx = so.first + (uint64_t)s * so.stride;
            guide_chain<ENV, DUMP>(S, A, G, px, py, A.samples[idx], idx, sc);
        }
    }
}

}  // namespace nd
