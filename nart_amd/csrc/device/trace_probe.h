// Test hook: the traversal entry points of the render kernels on caller-supplied rays against the
// context's device scene (nart_hip_trace, include/nart_hip.h: the records and variants are documented
// there).  One lane per ray, 256-lane blocks.  Like probe.h it only calls the functions the render
// kernels call (traverse, stage_nodes, trav_begin / trav_step / oc_resolve, traverse_packet,
// fill_isect) with the stack and node pointers those kernels form, and no render path launches it.
#pragma once

#include "../../../include/nart_hip.h"
#include "kernels.h"

namespace nd {

struct TraceProbeArgs {
    const float* in = nullptr;  // n records of NART_TRACE_IN_WORDS
    uint32_t* out = nullptr;    // n records of NART_TRACE_OUT_WORDS
    uint32_t n = 0;
    uint32_t stack_depth = 0;   // levels of the context's traversal stack
    uint32_t lds_nodes = 0;     // top BVH nodes staged in LDS behind the stack
    uint32_t sk = 0;            // short stack: levels in LDS (RenderArgs::stack_lds)
    int2* gstack = nullptr;     // short stack: (stack_depth - sk) entries per thread (RenderArgs::gstack)
};

struct TraceQuery {
    Ray ray;
    float tmax;
    bool any;
};
ND TraceQuery trace_probe_in(const TraceProbeArgs& P, uint32_t i) {
    const float4* q = reinterpret_cast<const float4*>(P.in + (size_t)i * NART_TRACE_IN_WORDS);
    const float4 a = q[0], b = q[1];
    TraceQuery t;
    t.ray = make_ray(F3(a.x, a.y, a.z), F3(b.x, b.y, b.z));
    t.tmax = a.w;
    t.any = __float_as_uint(b.w) == (uint32_t)NART_TRACE_ANY;
    return t;
}

template <bool COUNT>
ND void trace_probe_out(const DScene& S, const TraceProbeArgs& P, uint32_t i, const TraceQuery& q, float bt, uint32_t bg,
                        const TraceCounters& cnt) {
    uint32_t w[NART_TRACE_OUT_WORDS];
#pragma unroll
    for (int k = 0; k < NART_TRACE_OUT_WORDS; ++k) w[k] = 0u;
    if (q.any) {
        w[0] = bg != NO_HIT ? 1u : 0u;
    } else {
        w[0] = bg;
        w[1] = __float_as_uint(bt);
    }
    if (COUNT) {
        w[2] = cnt.nodes;
        w[3] = cnt.tris;
        w[4] = cnt.oc_checks;
        w[5] = cnt.oc_replays;
    }
    if (!q.any && bg != NO_HIT) {
        Isect is;
        fill_isect(S, q.ray, bg, is);
        const float f[17] = {is.p.x, is.p.y, is.p.z, is.gn.x, is.gn.y, is.gn.z, is.sn.x, is.sn.y, is.sn.z,
                             is.dpds.x, is.dpds.y, is.dpds.z, is.dpdt.x, is.dpdt.y, is.dpdt.z, is.st.x, is.st.y};
#pragma unroll
        for (int k = 0; k < 17; ++k) w[6 + k] = __float_as_uint(f[k]);
        w[23] = is.meshID;
        w[24] = is.priority;
        w[25] = is.mat;
    }
    uint4* o = reinterpret_cast<uint4*>(P.out + (size_t)i * NART_TRACE_OUT_WORDS);
#pragma unroll
    for (int k = 0; k < NART_TRACE_OUT_WORDS / 4; ++k) o[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

// traverse<> on the [depth][lane] LDS stack, with k_render's staged nodes behind it (lds_nodes = 0: none,
// as k_guide and k_primary call it)
template <bool COUNT>
__global__ __launch_bounds__(256) void k_trace_probe(DScene S, TraceProbeArgs P) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    float4* s_nodes = reinterpret_cast<float4*>(s_dyn + 2 * P.stack_depth * blockDim.x);
    stage_nodes(S, s_nodes, P.lds_nodes);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    int* sc = reinterpret_cast<int*>(reinterpret_cast<int2*>(s_dyn) + threadIdx.x);  // [depth][lane] int2
    const TraceQuery q = trace_probe_in(P, i);
    TraceCounters cnt = {0u, 0u, 0u, 0u};
    float bt;
    uint32_t bg;
    traverse<COUNT>(S, q.ray, q.tmax, q.any, bt, bg, sc, nullptr, (int)blockDim.x, cnt, P.lds_nodes ? s_nodes : nullptr,
                    (int)P.lds_nodes);
    trace_probe_out<COUNT>(S, P, i, q, bt, bg, cnt);
}

// the resumable form as k_render_rq runs it: its stack, node and global-column pointers
template <bool COUNT, bool ROT, bool SHORT>
__global__ __launch_bounds__(256) void k_trace_probe_step(DScene S, TraceProbeArgs P) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    const int tid = threadIdx.x;
    const int stride = blockDim.x;
    int2* s_stack = reinterpret_cast<int2*>(s_dyn);
    const uint32_t sk = SHORT ? P.sk : P.stack_depth;
    float4* s_nodes = reinterpret_cast<float4*>(s_stack + sk * blockDim.x);
    stage_nodes<ROT>(S, s_nodes, P.lds_nodes);
    const int nl = (int)P.lds_nodes;
    const uint32_t gid = blockIdx.x * blockDim.x + tid;
    if (gid >= P.n) return;
    int* sc = reinterpret_cast<int*>(s_stack + tid);
    int2* gstk = SHORT ? P.gstack + (size_t)gid * (P.stack_depth - sk) : nullptr;
    const TraceQuery q = trace_probe_in(P, gid);
    TraceCounters cnt = {0u, 0u, 0u, 0u};
    Trav tq;
    trav_begin(S, q.ray, q.tmax, q.any, tq);
    bool fin = !S.geometry_visible;
    while (!fin) fin = trav_step<COUNT, ROT, SHORT>(S, q.ray, tq, sc, gstk, stride, cnt, s_nodes, nl, (int)sk);
    float bt = tq.bestT;
    uint32_t bg = tq.bestG;
    if (S.geometry_visible)
        oc_resolve<COUNT>(S, q.ray, tq.tmax, tq.any, tq.risky, tq.bestInfo, fminf(tq.t2, oc_cull(S, tq.bestT)), bt, bg, cnt);
    trace_probe_out<COUNT>(S, P, gid, q, bt, bg, cnt);
}

// traverse_packet: a wave = 64 consecutive records, on k_primary_px's wave stacks
template <bool COUNT>
__global__ __launch_bounds__(256) void k_trace_probe_packet(DScene S, TraceProbeArgs P) {
    extern __shared__ __attribute__((aligned(16))) int s_dyn[];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint4* wstk = reinterpret_cast<uint4*>(s_dyn) + wave * P.stack_depth;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const TraceQuery q = trace_probe_in(P, i);
    TraceCounters cnt = {0u, 0u, 0u, 0u};
    float bt;
    uint32_t bg;
    traverse_packet<COUNT>(S, q.ray, q.tmax, bt, bg, wstk, cnt);
    trace_probe_out<COUNT>(S, P, i, q, bt, bg, cnt);
}

}  // namespace nd
