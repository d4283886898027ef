// C-ABI of the MI355X render path (include/nart_hip.h): context creation (scene upload, BVH
// build, light precomputation) and the Render()-equivalent launch sequence.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>  // types only: RCCL is loaded at run time by the multi-device context

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nart_hip.h"
#include "device/adaptive.h"
#include "device/cascade.h"
#include "device/halves.h"
#include "device/denoise_cross.h"
#include "device/cost.h"
#include "device/denoise.h"
#include "device/denoise_parts.h"
#include "device/depthcut.h"
#include "device/guide.h"
#include "device/lbvh.h"
#include "device/lightgroup.h"
#include "device/matte.h"
#include "device/probe.h"
#include "device/scene_probe.h"
#include "device/trace_probe.h"
#include "device/volume.h"
#include "host/bucket_batch.h"
#include "host/bvh_build.h"
#include "host/denoise_parts_plan.h"
#include "host/denoise_passes.h"
#include "host/device_buf.h"
#include "host/frame_plan.h"
#include "host/latin_plan.h"
#include "host/path_build.h"
#include "host/path_schedule.h"
#include "host/splat_plan.h"
#include "host/stage_params.h"

using namespace nd;

// The HIP backend of host/device_buf.h: the only calls that allocate or free device memory and events.
struct HipBackend {
    using event_t = hipEvent_t;
    static int malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static int free(void* p) { return hipFree(p); }
    static int get_device(int* d) { return hipGetDevice(d); }
    static int set_device(int d) { return hipSetDevice(d); }
    static int event_create(event_t* e) { return hipEventCreate(e); }
    static int event_destroy(event_t e) { return hipEventDestroy(e); }
};
using Buf = DevBuf<HipBackend>;
using Event = DevEvent<HipBackend>;

// A stream of a multi-device context, destroyed with its device current.
struct Stream {
    hipStream_t s = nullptr;
    int device = 0;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)), device(o.device) {}
    ~Stream() {
        if (!s) return;
        OnDevice<HipBackend> on(device);
        hipStreamDestroy(s);
    }
};

// The events around the launches of a denoise (run_denoise_passes: one before the first launch, one
// after each) and the last run's device times by slot (host/denoise_passes.h, DN_SLOT_*).
struct DenoiseTimes {
    Event ev[DN_EVENT_BUDGET];
    double ms[DN_SLOTS] = {};
};

struct nart_ctx {
    int device = 0;
    std::string err;
    DScene scene;
    uint32_t stack_depth = 1;
    uint32_t num_nodes = 0;
    int variant = 0;
    // 3 four pixels per lane (default), 2/1/0 one pixel per lane
    int splat_mode = -1;  // -1: automatic (plan_splat)
    bool counters = false;
    bool has_env = false;  // scene has an environment light (selects the k_render build)
    uint32_t features = FT_ALL;  // scene feature mask (scene_features): selects the k_render_rq build
    bool specialize = true;      // nart_hip_set_specialize: scene-specialised path kernels
    uint32_t fm_used = FT_ALL;   // the feature mask of the last path-kernel build launched
    bool lean = true;            // the three-waves-per-SIMD build where it fits (plan_build)
    // scene buffers
    Buf d_nodes, d_tri_isect, d_tri_perm, d_tris, d_tri_mesh, d_meshes;
    Buf d_mesh_eta;  // DScene::mesh_eta
    Buf d_mats, d_lights, d_texs, d_tex_pool, d_envs, d_density;
    Buf d_oc_nodes, d_oc_chunks, d_oc_tris, d_tri_leaf;  // reference octree (octree.h)
    Buf d_oc_lock, d_oc_heap;                            // replay heap pool
    std::vector<Buf> env_bufs;                           // Piecewise2DDistribution tables
    // work buffers of a batch, in three groups that each share a capacity counted in slots, samples
    // and buckets (ensure)
    Buf d_slot_xy;  // uint32_t
    Buf d_slot_so;  // SlotSO [slot] {first sample index, sample stride} (RenderArgs::slot_so)
    Buf d_rng;      // uint32_t
    Buf d_samples;  // float2
    Buf d_L;        // float4
    Buf d_prim;     // uint32_t camera-ray hits per sample (k_primary), same indexing as d_samples
    Buf d_bucket_ids, d_bucket_base;  // uint32_t
    size_t cap_slots = 0, cap_samples = 0, cap_buckets = 0;
    Buf d_table;     // float filter table and thresholds (plan_splat)
    Buf d_lut;       // splat filter-weight cells (splat_lut)
    Buf d_counters;  // unsigned long long (counter_buffer)
    // around a batch's kernels (render_buckets); ev_primary is recorded by launch_render
    Event ev_latin0, ev_path0, ev_primary, ev_path1, ev_splat1;
    bool primary_ran = false;  // the last dispatch launched k_primary (ev_primary recorded)
    bool prim_valid = false;   // d_prim holds the current batch's camera-ray hits (first-hit AOVs)
    bool rows_pixel_major = false;  // d_slot_so as last written: every slot's samples a contiguous row (stride 1)
    // around each pass of a batch after the beauty's splat (render_buckets; host/frame_plan.h PassKind)
    Event ev_pass[PASS_SLOTS][2];
    // around the error and scatter kernels of an adaptive level (render_buckets_adaptive)
    Event ev_ad[2];
    // around the cascade's reweighting (cascade_device) and the mattes' ranking (matte_rank_device)
    Event ev_cas[2], ev_mat[2];
    // the last cascade call's times: split + layer splats, reweighting; the last matte call's: plane
    // passes, ranking.  [0] is kept on the caller's context, [1] on the first device's (first_device)
    double cas_ms[2] = {0.0, 0.0};
    double mat_ms[2] = {0.0, 0.0};
    uint32_t num_meshes = 0, num_materials = 0;  // the scene's: the id counts of the two matte kinds
    uint32_t num_textures = 0;  // the scene's: nart_hip_scene_eval checks a record's texture index against it
    std::vector<DLight> lights;      // the host's copy of DScene::lights, and {w, h} of DScene::envs[k]:
    std::vector<uint32_t> env_dims;  // nart_hip_scene_eval checks a record's coordinates against them
    // light groups: the group of every light, uploaded by the call (set_light_groups); events around a
    // batch's group splats (render_buckets) and the mix (light_mix_device); the last call's times: group
    // splats ([0] on the caller's context), mix ([1] on the first device's)
    Buf d_light_group;
    Event ev_lg[2], ev_mix[2];
    double lg_ms[2] = {0.0, 0.0};
    // depth cuts: the cuts of the call (set_depth_cuts; they travel in the kernel arguments), n_depth_cuts
    // of them; their splats share ev_lg; events around the layers (depth_layers_device); the last call's
    // times: cut splats ([0] on the caller's context), layers ([1] on the first device's)
    uint32_t depth_cuts[8] = {0, 0, 0, 0, 0, 0, 0, 0}, n_depth_cuts = 0;
    Event ev_layers[2];
    double dc_ms[2] = {0.0, 0.0};
    // cost image: the grid of traced pixels a cost frame reduces its batches' records into (uint4 per
    // pixel, sized and zeroed by render_cost at the start of the frame, one per device), its size; events
    // around a batch's reduce (render_buckets) and around k_cost_image (cost_image_device); the last
    // call's times: reduce ([0] on the caller's context), image ([1] on the first device's)
    Buf d_cost_grid;
    uint32_t cost_grid_w = 0, cost_grid_h = 0;
    Event ev_cost[2], ev_cost_img[2];
    double cost_ms[2] = {0.0, 0.0};
    // denoiser (denoise_device): work buffers over the cropped image, the four device images of
    // nart_hip_denoise / nart_hip_render_denoised (five with the moment image)
    Buf d_dn, d_dn_img;
    // the last run of the denoiser, of the cross-filtered denoiser (denoise_cross_device) and of the
    // denoised parts (denoise_parts_device; each time summed over the chunks), on the first device's
    // context.  The latter two's images and work buffers are temporaries of the call.
    DenoiseTimes dn, dnx, dnp;
    // on the caller's context: the render_ms of the guides frame of the last whole-frame parts call
    double dnp_guides_ms = 0.0;
    uint32_t sched = 0;        // NART_SCHED_* bits of the current render (nart_render_stats::schedule)
    // path-kernel scheduling buffers (ensure_queue, ensure_ilist, ensure_gstack; launch_render,
    // dispatch_volume): the queue group shares a capacity counted in queue entries
    Buf d_queue, d_cost, d_keys[2], d_vals[2], d_qhead;  // uint32_t
    Buf d_sort_tmp;
    size_t cap_queue = 0;
    Buf d_ilist;   // dielectric-list columns beyond ILIST_REG (bounces > ILIST_REG)
    Buf d_gstack;  // lean build: traversal-stack levels beyond the LDS (RenderArgs::gstack)
    // multi-device context (nart_hip_create_multi, host/multi_gpu.h): one single-device
    // sub-context per listed device; device 0 gathers and combines
    std::vector<nart_ctx*> subs;
    std::vector<int> devs;
    std::vector<Stream> streams;
    std::vector<Buf> sub_tiles;
    std::vector<ncclComm_t> comms;
    bool gather_rccl = false;
    // RCCL requested implicitly (distinct devices) but unavailable: device-copy gather instead
    bool gather_fallback = false;
    // an RCCL gather failed: the communicator's state is unknown, every later render of this
    // context returns NART_E_RCCL (destroy it and create a new one)
    bool rccl_broken = false;
    int debug_fault = 0;     // nart_hip_debug_fault (tests only)
    uint32_t mem_share = 1;  // contexts of one multi-device context sharing this device ordinal
    // acceleration structure: built on the device (NART_BVH_BUILD=device) or the host; build time
    bool bvh_on_device = false;
    double bvh_ms = 0.0;
    uint32_t num_leaf_tris = 0;
    int32_t root_code = -1;  // the traversal's root (DScene::root), kept for nart_hip_context_bvh_dump
    float bvh_pad = 0.f;     // what the child boxes were grown by
    // whole frames (render_frame, render_multi): gathered tiles, tiles by bucket id, image, slab map
    Buf d_gather, d_byid, d_image, d_slab_map;
};

namespace {

int fail(nart_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    return code;
}
// On failure the error is also cleared from HIP's sticky last-error state, so that a context whose
// call failed (e.g. an allocation) renders normally afterwards.
#define HIPCHK(call)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (void)hipGetLastError();                                                             \
            return fail(ctx, e_ == hipErrorOutOfMemory ? NART_E_OOM : NART_E_HIP,                \
                        std::string(#call ": ") + hipGetErrorString(e_));                        \
        }                                                                                        \
    } while (0)

// Run-time switches, all read here.  Fallbacks a deployment can need: NART_BATCH_BYTES (per-batch
// memory budget), NART_BVH_BUILD=device, NART_GATHER=rccl|copy.  The others are test hooks that
// force one scheduling or kernel path of an otherwise automatic choice so that the GPU parity suite
// covers it (tests/test_gpu_*.py; DESIGN.md section 2 lists them); none changes an image.
const char* env_opt(const char* name) { return std::getenv(name); }
double env_num(const char* name, double def) {
    const char* e = env_opt(name);
    return e && *e ? std::atof(e) : def;
}

// The one way a device buffer of a context or a call grows: `buf` holds at least `bytes` on `device`
// afterwards (DevBuf::reserve: only grows, frees before it allocates, empty after a failure).  A
// failed allocation leaves no sticky error behind, so that the next render's hipGetLastError() does
// not report it and the context renders normally afterwards.
int reserve(nart_ctx* ctx, Buf& buf, int device, size_t bytes, const char* what) {
    const hipError_t e = (hipError_t)buf.reserve(device, bytes);
    if (e == hipSuccess) return NART_OK;
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? NART_E_OOM : NART_E_HIP,
                std::string("hipMalloc ") + what + " (" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
}
// The same for a group of the context's buffers that shares the capacity `cap` (reserve_group).
int reserve(nart_ctx* ctx, size_t& cap, size_t count, std::initializer_list<GroupItem<HipBackend>> items) {
    return reserve_group(cap, count, items, [ctx](Buf& buf, size_t bytes, const char* what) {
        return reserve(ctx, buf, ctx->device, bytes, what);
    });
}

// `e` recorded on `st`, created on its first use.
hipError_t record(Event& e, hipStream_t st) {
    hipEvent_t h = nullptr;
    const int err = e.get(&h);
    return err ? (hipError_t)err : hipEventRecord(h, st);
}

template <typename T>
int upload(nart_ctx* ctx, Buf& dst, const T* src, size_t count, const char* what) {
    if (int rc = reserve(ctx, dst, ctx->device, sizeof(T) * (count ? count : 1), what)) return rc;
    if (count) HIPCHK(hipMemcpy(dst.as<T>(), src, sizeof(T) * count, hipMemcpyHostToDevice));
    return NART_OK;
}

// The context that does the work of one device for ctx: device 0's sub-context of a multi-device
// context (it combines, holds the images and runs the stages over them), else ctx itself.
nart_ctx* first_device(nart_ctx* ctx) { return ctx->subs.empty() ? ctx : ctx->subs[0]; }
const nart_ctx* first_device(const nart_ctx* ctx) { return ctx->subs.empty() ? ctx : ctx->subs[0]; }
// rc of a call made on first_device(ctx): its error is re-raised on the caller's context.
int forwarded(nart_ctx* ctx, int rc) { return rc && !ctx->subs.empty() ? fail(ctx, rc, ctx->subs[0]->err) : rc; }

// The device time in ms of what `launch` (returning a code) puts on `st`, between the event pair
// `ev`; waits for it.
template <typename Launch>
int timed(nart_ctx* ctx, Event (&ev)[2], hipStream_t st, double* ms, Launch&& launch) {
    HIPCHK(record(ev[0], st));
    if (int rc = launch()) return rc;
    HIPCHK(record(ev[1], st));
    HIPCHK(hipEventSynchronize(ev[1].handle()));
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, ev[0].handle(), ev[1].handle()));
    *ms = t;
    return NART_OK;
}

// How the images of p lie in memory: the cropped window W x H inside totalW x totalH pixels of five
// floats (nart_pixel), the filter's border fb around it.
struct ImageLayout {
    nart_session_geometry g;
    uint32_t W, H;
    size_t img_floats, img_bytes;
    explicit ImageLayout(const nart_render_params* p) : W(p->image_width), H(p->image_height) {
        nart_session_geometry_of(p, &g);
        img_floats = (size_t)g.total_width * g.total_height * 5;
        img_bytes = img_floats * sizeof(float);
    }
    // into the kernel arguments of a stage over whole images (device/denoise.h, cascade.h, matte.h)
    template <typename Args>
    void fill(Args& a) const {
        a.W = W;
        a.H = H;
        a.totalW = g.total_width;
        a.totalH = g.total_height;
        a.fb = g.filter_bounds;
    }
};

// Images back to back in a buffer on ctx's device (a single-device context; errors go to it).
struct Images {
    nart_ctx* ctx;
    ImageLayout layout;
    float* base = nullptr;
    Images(nart_ctx* c, const nart_render_params* p) : ctx(c), layout(p) {}
    // over `buf`, grown to hold n images; makes the device current for what follows
    int in(Buf& buf, size_t n, const char* what) {
        HIPCHK(hipSetDevice(ctx->device));
        if (int rc = reserve(ctx, buf, ctx->device, n * layout.img_bytes, what)) return rc;
        base = buf.as<float>();
        return NART_OK;
    }
    float* at(size_t i) const { return base + i * layout.img_floats; }
    int upload(size_t i, const nart_pixel* src, size_t k = 1) const {  // k host images to image i onwards
        if (k) HIPCHK(hipMemcpy(at(i), src, k * layout.img_bytes, hipMemcpyHostToDevice));
        return NART_OK;
    }
    int download(size_t i, nart_pixel* dst, size_t k = 1) const {  // k images from image i to the host
        if (k) HIPCHK(hipMemcpy(dst, at(i), k * layout.img_bytes, hipMemcpyDeviceToHost));
        return NART_OK;
    }
    int zero_async(size_t i, size_t k, hipStream_t st) const {
        HIPCHK(hipMemsetAsync(at(i), 0, k * layout.img_bytes, st));
        return NART_OK;
    }
};

// Feature mask of a scene (FT_*, path.h): every material kind, light kind, textured pattern and
// normal map the scene's records hold (a glass material's normal map is ignored, as the device
// record drops it: glassmaterial.cpp:3-9).  A path kernel built for a mask covering it compiles
// only that code; unknown kinds give FT_ALL (the generic build).
uint32_t scene_features(const nart_scene_blob* blob) {
    uint32_t f = 0;
    auto ptn = [&](const nart_pattern& p) {
        if (p.type != NART_PTN_CONSTANT) f |= FT_TEX;
    };
    for (uint32_t i = 0; i < blob->num_materials; ++i) {
        const nart_material& m = blob->materials[i];
        switch (m.type) {
            case NART_MAT_LAMBERT: f |= FT_LAMBERT; break;
            case NART_MAT_SPECULAR: f |= FT_SPECMAT; break;
            case NART_MAT_GLASS: f |= FT_GLASS; break;
            case NART_MAT_GLOSSY: f |= FT_GLOSSY; break;
            case NART_MAT_PLASTIC: f |= FT_PLASTIC; break;
            default: return FT_ALL;
        }
        for (const nart_pattern* p : {&m.rho_d, &m.rho_s, &m.tau, &m.eta, &m.alpha}) ptn(*p);
        if (m.type != NART_MAT_GLASS && m.has_normal) {
            f |= FT_NMAP;
            ptn(m.normal);
        }
    }
    for (uint32_t l = 0; l < blob->num_lights; ++l) {
        const nart_light& L = blob->lights[l];
        switch (L.type) {
            case NART_LIGHT_DISK: f |= FT_DISK; break;
            case NART_LIGHT_RING: f |= FT_RING; break;
            case NART_LIGHT_ENVIRONMENT: f |= FT_ENV; break;
            default: return FT_ALL;
        }
        ptn(L.Le);
    }
    return f;
}

DPattern dpat(const nart_pattern& p) {
    DPattern d;
    d.type = p.type;
    d.tex = p.texture;
    d.rough = p.is_roughness;
    d.v[0] = p.value[0];
    d.v[1] = p.value[1];
    d.v[2] = p.value[2];
    return d;
}

// Per-call light constants of disklight.cpp / ringlight.cpp, computed with the same float
// operations the reference executes on every call (vec4 * mat4 row-vector products).
DLight dlight(const nart_light& L) {
    DLight d;
    std::memset(&d, 0, sizeof(d));
    d.type = L.type;
    d.radius = L.radius;
    d.inner = L.inner_radius;
    d.intensity = L.intensity;
    d.Le = dpat(L.Le);
    std::memcpy(d.m, L.m, sizeof(d.m));
    f4 c = vec_mul_mat(F4(0.f, 0.f, 0.f, 1.f), L.m);
    f4 n = vec_mul_mat(F4(0.f, 0.f, -1.f, 0.f), L.m);
    f4 u = vec_mul_mat(F4(1.f, 0.f, 0.f, 0.f), L.m);
    f4 v = vec_mul_mat(F4(0.f, 1.f, 0.f, 0.f), L.m);
    d.center[0] = c.x; d.center[1] = c.y; d.center[2] = c.z;
    d.n[0] = n.x; d.n[1] = n.y; d.n[2] = n.z;
    d.D = dot(F3(c.x, c.y, c.z), F3(n.x, n.y, n.z));
    d.axu[0] = u.x; d.axu[1] = u.y; d.axu[2] = u.z; d.axu[3] = u.w;
    d.axv[0] = v.x; d.axv[1] = v.y; d.axv[2] = v.z; d.axv[3] = v.w;
    const float pi = ND_PI;
    if (L.type == NART_LIGHT_RING)
        d.pdf_area = 1.f / (pi * (1.f - ((L.inner_radius * L.inner_radius) / (L.radius * L.radius))) * L.radius * L.radius);
    else
        d.pdf_area = 1.f / (pi * L.radius * L.radius);
    d.r2 = L.radius * L.radius;
    d.ri2 = L.inner_radius * L.inner_radius;
    d.inner_ratio = L.inner_radius / L.radius;
    d.env = -1;
    return d;
}

// Guide table of one BinarySearch range v[0, n) (path.h guided_search): for each of the K cells of
// values [c/K, (c+1)/K) the range [ub(c/K), ub(last float of the cell)] of the upper bound (first
// index with v[j] > value), 16 bits each.  Only for non-decreasing, NaN-free ranges of < 2^16
// entries; otherwise false and the device runs the full search.
bool env_guide(const float* v, uint32_t n, uint32_t* out) {
    const uint32_t K = NART_ENV_GUIDE_K;
    if (n > 65535u) return false;
    for (uint32_t j = 0; j + 1 < n; ++j)
        if (!(v[j] <= v[j + 1])) return false;
    if (n && v[0] != v[0]) return false;
    auto ub = [&](float x) { return (uint32_t)(std::upper_bound(v, v + n, x) - v); };
    for (uint32_t c = 0; c < K; ++c) {
        const float lo = (float)c / (float)K;
        const float hi = c + 1 == K ? INFINITY : std::nextafter((float)(c + 1) / (float)K, 0.f);
        out[c] = ub(lo) | (ub(hi) << 16);
    }
    return true;
}

// Piecewise2DDistribution of an environment texture (texturepattern.cpp:3-70): marginal pdf of
// the rows (top row last), conditional pdf per row, and their CDFs, with the reference's float
// operation order.  Built on the host once per context.
int build_env(nart_ctx* ctx, const nart_texture& t, DEnvDist& d) {
    const uint32_t W = t.width, H = t.height;
    std::vector<float> mpdf(H), cpdf((size_t)W * H), mcdf(H + 1), ccdf((size_t)W * H + H);
    auto texel = [&](uint32_t row, uint32_t i) {  // |r| + |g| + |b| of the flipped row
        const uint16_t* q = t.rgba + ((size_t)(H - row - 1) * W + i) * 4;
        return std::fabs(nart_half_to_float(q[0])) + std::fabs(nart_half_to_float(q[1])) +
               std::fabs(nart_half_to_float(q[2]));
    };
    const float invW = 1.f / (float)W, invH = 1.f / (float)H;
    float fInt = 0.f;
    for (uint32_t j = 0; j < H; ++j) {
        mpdf[j] = 0.f;
        for (uint32_t i = 0; i < W; ++i) mpdf[j] += texel(j, i);
        mpdf[j] *= invW;
        fInt += mpdf[j];
    }
    fInt *= invH;
    for (uint32_t j = 0; j < H; ++j) {
        if (mpdf[j] != 0.f) {
            for (uint32_t i = 0; i < W; ++i) {
                cpdf[(size_t)j * W + i] = texel(j, i);
                cpdf[(size_t)j * W + i] /= mpdf[j];
            }
        } else {
            for (uint32_t i = 0; i < W; ++i) cpdf[(size_t)j * W + i] = 1.f;
        }
    }
    const float invFInt = 1.f / fInt;
    for (uint32_t j = 0; j < H; ++j) mpdf[j] *= invFInt;
    mcdf[0] = 0.f;
    mcdf[H] = 1.f;
    for (uint32_t i = 1; i < H; ++i) mcdf[i] = mcdf[i - 1] + (mpdf[i - 1] * invH);
    for (uint32_t i = 0; i < H; ++i) {
        ccdf[(size_t)i * (W + 1)] = 0.f;
        ccdf[(size_t)i * (W + 1) + W] = 1.f;
    }
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 1; i < W; ++i)
            ccdf[(size_t)j * (W + 1) + i] = ccdf[(size_t)j * (W + 1) + i - 1] + (cpdf[(size_t)j * W + i - 1] * invW);
    // guide tables of the two searches (path.h guided_search): per cell of values [c/K, (c+1)/K)
    // the range [ub(c/K), ub(last float of the cell)] of the upper bound; built only over searched
    // ranges that are non-decreasing and NaN-free (otherwise the full search runs)
    const uint32_t K = NART_ENV_GUIDE_K;
    auto guide = env_guide;
    std::vector<uint32_t> mguide(K), cguide((size_t)K * H);
    bool guided = W <= 65535 && H <= 65535 && guide(mcdf.data(), H, mguide.data());
    for (uint32_t j = 0; guided && j < H; ++j) guided = guide(ccdf.data() + (size_t)j * (W + 1), W, cguide.data() + (size_t)j * K);
    // each table into a buffer of its own, kept by the context
    int rc = NART_OK;
    auto table = [&](const auto& v, const char* what) {
        ctx->env_bufs.emplace_back();
        if (!rc) rc = upload(ctx, ctx->env_bufs.back(), v.data(), v.size(), what);
        return ctx->env_bufs.back().as<std::remove_reference_t<decltype(v[0])>>();  // const float / uint32_t
    };
    d.mpdf = table(mpdf, "environment row pdf");
    d.cpdf = table(cpdf, "environment column pdfs");
    d.mcdf = table(mcdf, "environment row cdf");
    d.ccdf = table(ccdf, "environment column cdfs");
    d.mguide = guided ? table(mguide, "environment row guide") : nullptr;
    d.cguide = guided ? table(cguide, "environment column guides") : nullptr;
    d.w = W;
    d.h = H;
    d.invW = invW;
    d.invH = invH;
    return rc;
}

// Camera medium: density grid upload + the width-1 MajorantGrid (media.cpp:47-130) on the host.
int build_medium(nart_ctx* ctx, const nart_medium& bm, DMedium& m) {
    std::memset(&m, 0, sizeof(m));
    if (!bm.present) return NART_OK;
    m.present = 1;
    m.rx = (uint8_t)bm.res[0];  // DensityGrid(uint8_t, uint8_t, uint8_t, ...) (scene.cpp:866-868)
    m.ry = (uint8_t)bm.res[1];
    m.rz = (uint8_t)bm.res[2];
    if (m.rx < 2 || m.ry < 2 || m.rz < 2)
        return fail(ctx, NART_E_UNSUPPORTED, "density grids need >= 2 points per axis (DensityGrid::LookUp reads past the grid)");
    for (int i = 0; i < 3; ++i) {
        m.bmin[i] = bm.bounds_min[i];
        m.bmax[i] = bm.bounds_max[i];
        m.Le[i] = bm.Le[i];
    }
    m.sigma_a = bm.sigma_a;
    m.sigma_s = bm.sigma_s;
    const uint32_t npts = bm.res[0] * bm.res[1] * bm.res[2];
    m.density = bm.density;  // host view for the majorant search below
    const float sigma_maj = bm.sigma_a + bm.sigma_s;
    const float mx = ((float)m.rx - 1.f) / 1.f, my = ((float)m.ry - 1.f) / 1.f, mz = ((float)m.rz - 1.f) / 1.f;
    auto u8min = [](uint32_t a, uint32_t b) { return b < a ? b : a; };
    const uint32_t x1 = u8min((uint8_t)(uint32_t)std::ceil(mx), m.rx);
    const uint32_t y1 = u8min((uint8_t)(uint32_t)std::ceil(my), m.ry);
    const uint32_t z1 = u8min((uint8_t)(uint32_t)std::ceil(mz), m.rz);
    float majorant = 0.f;
    for (uint32_t k = 0; k < z1; ++k)
        for (uint32_t j = 0; j < y1; ++j)
            for (uint32_t i = 0; i < x1; ++i) majorant = gmax(majorant, dg_at(m, m.density, i, j, k));
    for (int c = 0; c < 8; ++c)
        majorant = gmax(majorant, dg_lookup(m, m.density, F3((c & 4) ? 1.f : 0.f, (c & 2) ? 1.f : 0.f, (c & 1) ? 1.f : 0.f)));
    m.maj[0] = majorant * sigma_maj;
    m.maj[1] = sigma_maj;
    for (int i = 0; i < 3; ++i) {
        m.maj[2 + i] = bm.bounds_min[i];
        m.maj[5 + i] = bm.bounds_max[i];
    }
    // exact reciprocals of power-of-two divisors (x / 2^k and x * 2^-k round the same real value)
    auto pow2 = [](float x, float& inv) {
        int e = 0;
        if (!(x > 0.f) || !std::isfinite(x) || std::frexp(x, &e) != 0.5f) return false;
        inv = 1.f / x;
        return std::isnormal(inv) && std::frexp(inv, &e) == 0.5f;
    };
    for (int i = 0; i < 3; ++i)
        if (pow2(m.bmax[i] - m.bmin[i], m.inv_bs[i])) m.bs_pow2 |= 1u << i;
    for (int j = 0; j < 8; ++j)
        if (pow2(m.maj[j], m.inv_maj[j])) m.maj_pow2 |= 1u << j;
    if (m.rx == 2 && m.ry == 2 && m.rz == 2) {
        m.grid2 = 1;
        for (int i = 0; i < 8; ++i) m.dens8[i] = bm.density[i];
    }
    int rc = upload(ctx, ctx->d_density, bm.density, npts, "density grid");
    m.density = ctx->d_density.as<const float>();
    return rc;
}

int check_params(nart_ctx* ctx, const nart_render_params* p) {
    if (!p) return fail(ctx, NART_E_INVALID, "null params");
    if (p->integrator != NART_INTEGRATOR_PATH && p->integrator != NART_INTEGRATOR_VOLUME)
        return fail(ctx, NART_E_INVALID, "unknown integrator");
    if (!p->image_width || !p->image_height || !p->bucket_size || !p->spp)
        return fail(ctx, NART_E_INVALID, "imageWidth, imageHeight, bucketSize and spp must be > 0");
    if (!(p->filter_width > 0.f)) return fail(ctx, NART_E_INVALID, "filterWidth must be > 0");
    if (p->integrator == NART_INTEGRATOR_PATH && p->bounces > 32)
        return fail(ctx, NART_E_UNSUPPORTED, "bounces > 32 not supported by the path integrator");
    if (ctx->scene.num_lights == 0)
        return fail(ctx, NART_E_INVALID, "scene has no lights (reference throws in Scene::GetLight)");
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    if (g.total_width > 65535 || g.total_height > 65535) return fail(ctx, NART_E_UNSUPPORTED, "image too large");
    return NART_OK;
}

// Per-sample state of one batch (LatinSquare sample, radiance, camera hit: 28 B per sample).  An
// MI355X holds 288 GB, so by default a batch may take half of the device memory free at the call
// (plus what this context already holds for it), at least 16 GiB: whole frames up to 4K x 512 spp
// (119 GB) render in one batch -- fewer launch tails than the former fixed 16 GiB (C5 469 -> 413
// ms, C4 5.27 -> 4.43 s per frame; profiles/r03a_bb_c4.log, r03a_bb_c5_s*.log).  NART_BATCH_BYTES
// overrides.  A cascade or half-buffer call (nart_hip_render_cascade, nart_hip_render_halves) holds a
// second record buffer while it runs: extra_per_sample = 16, 44 B per sample (FramePlan::record_bytes
// has every frame's figure); a plain call passes 0 and sees what it saw before.
size_t batch_slot_limit(const nart_ctx* ctx, uint32_t spp, size_t extra_per_sample = 0) {
    size_t budget = (size_t)16 << 30;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t held = ctx->cap_samples * (sizeof(float2) + sizeof(float4) + sizeof(uint32_t));
        budget = std::max(budget, (free_b + held) / 2);
        // sub-contexts that share an ordinal (a multi-device rehearsal) render concurrently and
        // each sees the same free memory: split the budget between them
        budget /= std::max<uint32_t>(1, ctx->mem_share);
    } else {
        (void)hipGetLastError();
    }
    if (const char* e = env_opt("NART_BATCH_BYTES")) budget = (size_t)std::strtoull(e, nullptr, 10);
    size_t per = 8 + (size_t)spp * (sizeof(float2) + sizeof(float4) + sizeof(uint32_t) + extra_per_sample);
    size_t n = budget / per;
    return n < 256 ? 256 : n;
}

// Work buffers for a batch: three groups, each sharing a capacity counted in slots, samples and
// buckets (batch_slot_limit reads cap_samples).
int ensure(nart_ctx* ctx, size_t slots, uint32_t spp, size_t buckets) {
    const size_t samples = slots * spp;
    int rc = reserve(ctx, ctx->cap_slots, slots, {{&ctx->d_slot_xy, slots * 4, "slot pixels"},
                                                  {&ctx->d_slot_so, slots * sizeof(SlotSO), "slot sample table"},
                                                  {&ctx->d_rng, slots * 4, "slot RNG states"}});
    if (!rc)
        rc = reserve(ctx, ctx->cap_samples, samples, {{&ctx->d_samples, samples * sizeof(float2), "LatinSquare samples"},
                                                      {&ctx->d_L, samples * sizeof(float4), "per-sample radiance"},
                                                      {&ctx->d_prim, samples * sizeof(uint32_t), "camera-ray hits"}});
    if (!rc)
        rc = reserve(ctx, ctx->cap_buckets, buckets, {{&ctx->d_bucket_ids, buckets * 4, "bucket ids"},
                                                      {&ctx->d_bucket_base, buckets * 4, "bucket bases"}});
    return rc;
}

// The queue group as the scheduling steps and their kernels take it.
struct QueueBufs {
    uint32_t *queue, *cost, *keys[2], *vals[2], *qhead;
    void* sort_tmp;
    size_t sort_bytes;
    explicit QueueBufs(const nart_ctx* c)
        : queue(c->d_queue.as<uint32_t>()), cost(c->d_cost.as<uint32_t>()),
          keys{c->d_keys[0].as<uint32_t>(), c->d_keys[1].as<uint32_t>()},
          vals{c->d_vals[0].as<uint32_t>(), c->d_vals[1].as<uint32_t>()}, qhead(c->d_qhead.as<uint32_t>()),
          sort_tmp(c->d_sort_tmp.as<void>()), sort_bytes(c->d_sort_tmp.bytes()) {}
};

// Work-queue buffers of the megakernel scheduler (queue, cost probe, radix-sort scratch): one group
// of capacity n queue entries, complete once the sort scratch (sized from the others) is allocated.
int ensure_queue(nart_ctx* ctx, uint32_t n) {
    if (n <= ctx->cap_queue) return NART_OK;
    ctx->cap_queue = 0;
    ctx->d_sort_tmp.release();
    const size_t words = (size_t)n * 4;
    size_t cap = 0;
    if (int rc = reserve(ctx, cap, n, {{&ctx->d_queue, words, "work queue"}, {&ctx->d_cost, words, "probe costs"},
                                       {&ctx->d_keys[0], words, "sort keys"}, {&ctx->d_keys[1], words, "sort keys"},
                                       {&ctx->d_vals[0], words, "sort values"}, {&ctx->d_vals[1], words, "sort values"},
                                       {&ctx->d_qhead, 256, "queue head"}}))
        return rc;
    const QueueBufs q(ctx);
    size_t t1 = 0, t2 = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, q.keys[0], q.keys[1], q.vals[0], q.vals[1], (int)n, 0, 1));
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, t2, q.keys[0], q.keys[1], q.vals[0], q.vals[1],
                                              (int)((n + 63) / 64), 0, 32));
    if (int rc = reserve(ctx, ctx->d_sort_tmp, ctx->device, std::max(t1, t2) + 256, "sort scratch")) return rc;
    ctx->cap_queue = n;
    return NART_OK;
}

// The work counters of the path kernels (nart_hip_set_counters), allocated by a context's first render.
int counter_buffer(nart_ctx* ctx) {
    return reserve(ctx, ctx->d_counters, ctx->device, 24 * sizeof(unsigned long long), "work counters");
}

// The dielectric list's entries beyond ILIST_REG (bounces > ILIST_REG): one column per thread of
// the largest launch (whole 512-thread blocks over every slot).
int ensure_ilist(nart_ctx* ctx, RenderArgs& a) {
    const size_t lanes = ((size_t)a.n_slots + 511) / 512 * 512;
    a.ilist_stride = (uint32_t)lanes;
    const size_t bytes = lanes * (ILIST_MAX - ILIST_REG) * sizeof(uint2);
    const int rc = reserve(ctx, ctx->d_ilist, ctx->device, bytes, "dielectric lists");
    a.ilist_ext = ctx->d_ilist.as<uint2>();
    return rc;
}

// The lean build's traversal-stack levels beyond the LDS: `levels` entries per launched thread.
int ensure_gstack(nart_ctx* ctx, size_t threads, uint32_t levels, RenderArgs& a) {
    const int rc = reserve(ctx, ctx->d_gstack, ctx->device, threads * levels * sizeof(int2), "traversal stack columns");
    a.gstack = ctx->d_gstack.as<int2>();
    return rc;
}

// ---------------------------------------------------------------- megakernel scheduling
// host/path_schedule.h decides a launch's schedule (plan_path: the policy, its measurements and the
// knobs); the kernels below prepare what it asks for and launch_render executes it.

// Group (wave-sized run of 64 consecutive slots: a 16x4 strip of a bucket) costs, as keys of an
// ascending sort that puts the costliest group first; a partial last group always sorts last.
// per: cost entries per group (64: one per slot; fewer: the sampled probe, probe_sub).
__global__ void k_group_keys(const uint32_t* cost, uint32_t n, uint32_t* keys, uint32_t* vals, uint32_t per = 64) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t ng = (n + 63) / 64;
    if (g >= ng) return;
    uint64_t sum = 0;
    const uint32_t e = min(n, 64 * g + 64);
    if (per < 64) {  // a partial last group is keyed last below, whatever its entries hold
        if (e - 64 * g == 64)
            for (uint32_t i = per * g; i < per * g + per; ++i) sum += cost[i];
    } else {
        for (uint32_t i = 64 * g; i < e; ++i) sum += cost[i];
    }
    const uint32_t c = (uint32_t)min<uint64_t>(sum, 0xFFFFFFFEull);
    keys[g] = (e - 64 * g < 64) ? 0xFFFFFFFFu : 0xFFFFFFFEu - c;
    vals[g] = g;
}

// Two cost classes of groups for the wave-group refill order: keys[g] = 0 for the E costliest
// groups (ranks [0, E) of the cost-sorted list), 1 for the rest; vals = group ids in slot order,
// so a stable sort by the key keeps slot order inside each class.
__global__ void k_group_class(const uint32_t* sorted, uint32_t ng, uint32_t E, uint32_t* keys, uint32_t* vals) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ng) return;
    keys[sorted[r]] = r < E ? 0u : 1u;
    vals[r] = r;
}

// Pixel list of the sorted groups (group order, slot order inside a group).
__global__ void k_expand_groups(const uint32_t* groups, uint32_t n, uint32_t* pixels) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    pixels[r] = 64 * groups[r / 64] + r % 64;
}

// Mark the k*W costliest pixels (ranks [0, E) of the class-sorted list) for the 1-bit partition.
__global__ void k_flag_top(const uint32_t* sorted, uint32_t n, uint32_t E, uint32_t* flag) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    flag[sorted[r]] = r < E ? 1u : 0u;
}

// The probe-ordered pixel queue (device/queue_layout.h queue_entry): top = the pixels by cost class,
// rest = the others in slot order.
__global__ void k_build_queue(const uint32_t* top, const uint32_t* rest, uint32_t n, uint32_t W, uint32_t k,
                              uint32_t prio, uint32_t pairs, uint32_t half, uint32_t quad, uint32_t* queue) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= queue_length(n, W, k, pairs, quad)) return;
    const QueueEntry e = queue_entry(p, n, W, k, prio, pairs, half, quad);
    queue[p] = (e.top ? top : rest)[e.index] | e.flags;
}

// Sample-major bucket layout: slot `base + p` of a bucket of `cnt` traced pixels keeps sample s
// at base*spp + s*cnt + p (k_splat_col4's lanes then read neighbouring pixels' sample s from one
// line); pixel-major: at (base + p)*spp + s (k_splat_skew streams one pixel's samples).  One
// block per bucket of the batch.
__global__ void k_slot_table(const uint32_t* bucket_base, uint32_t nbk, uint32_t nslots, uint32_t spp, SlotSO* so,
                             bool pixel_major) {
    const uint32_t b = blockIdx.x;
    const uint32_t base = bucket_base[b], end = b + 1 < nbk ? bucket_base[b + 1] : nslots;
    for (uint32_t p = threadIdx.x; base + p < end; p += blockDim.x)
        so[base + p] = pixel_major ? SlotSO{(unsigned long long)(base + p) * spp, 1u, 0u}
                                   : SlotSO{(unsigned long long)base * spp + p, end - base, 0u};
}

__global__ void k_slot_rows(uint32_t n, uint32_t spp, SlotSO* so) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) so[i] = SlotSO{(unsigned long long)i * spp, 1u, 0u};
}

// Volume queue with the H costliest groups (sorted group ids, costliest first) spread S pixels per
// wave, the wave's other lanes idle (0xFFFFFFFF), then the remaining groups dense.
__global__ void k_sparse_groups(const uint32_t* groups, uint32_t n, uint32_t H, uint32_t S, uint32_t qlen,
                                uint32_t* queue) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= qlen) return;
    const uint32_t hot = H * (64u / S) * 64u;
    if (p < hot) {
        const uint32_t w = p / 64u, j = p % 64u, g = w / (64u / S), part = w % (64u / S);
        const uint32_t slot = 64u * groups[g] + part * S + j;
        queue[p] = (j < S && slot < n) ? slot : 0xFFFFFFFFu;
    } else {
        const uint32_t r = p - hot + 64u * H;  // rank in the dense group order
        queue[p] = 64u * groups[r / 64u] + r % 64u;
    }
}

__global__ void k_iota(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

// The wave-sized slot groups ordered by the probe costs in ctx->d_cost (`per` entries per group),
// costliest group first (ties keep slot order): group ids into ctx->d_vals[1], keys into d_keys[1];
// with `out`, their pixel list too.
int sort_groups_by_cost(nart_ctx* ctx, uint32_t n, uint32_t per, uint32_t* out, hipStream_t st) {
    const QueueBufs q(ctx);
    const uint32_t ng = (n + 63) / 64;
    hipLaunchKernelGGL(k_group_keys, dim3((ng + 255) / 256), dim3(256), 0, st, q.cost, n, q.keys[0],
                       q.vals[0], per);
    size_t tmp = q.sort_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(q.sort_tmp, tmp, q.keys[0], q.keys[1], q.vals[0],
                                              q.vals[1], (int)ng, 0, 32, st));
    if (out) hipLaunchKernelGGL(k_expand_groups, dim3((n + 255) / 256), dim3(256), 0, st, q.vals[1], n, out);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// Resident blocks of a kernel on the context's device (CUs x blocks per CU, at least one).  One
// query per dispatch and kernel: the callers pass the figure down.
int resident_blocks(nart_ctx* ctx, const void* kernel, int block, size_t lds, uint32_t* out) {
    int cus = 0, per_cu = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds));
    *out = (uint32_t)std::max(1, cus * std::max(per_cu, 1));
    return NART_OK;
}

// The knobs of the pure launch decisions (plan_path, plan_build, plan_volume), each read once per launch:
// the GPU tests set them between renders of one context.
void read_knobs(std::initializer_list<std::pair<const char*, Knob*>> all) {
    for (const auto& [name, knob] : all) {
        const char* e = env_opt(name);
        *knob = Knob{e != nullptr, e && *e, e && *e ? std::atof(e) : 0.0};
    }
}
SchedKnobs read_sched_knobs() {
    SchedKnobs k;
    read_knobs({{"NART_PRIMARY_PACKET", &k.primary_packet}, {"NART_RQ_PRIO", &k.rq_prio}, {"NART_RQ_PAIRS", &k.rq_pairs},
                {"NART_RQ_HALF", &k.rq_half}, {"NART_RQ_QUAD", &k.rq_quad}, {"NART_RQ_SETPRIO", &k.rq_setprio},
                {"NART_RQ_ORDER", &k.rq_order}, {"NART_RQ_TOPF", &k.rq_topf}, {"NART_PROBE_SUB", &k.probe_sub},
                {"NART_QUEUE_K", &k.queue_k}});
    return k;
}
void read_build_knobs(PathBuildIn& in) {
    read_knobs({{"NART_RQ_LDS_LIMIT", &in.rq_lds_limit}, {"NART_LEAN_STACK", &in.lean_stack}, {"NART_LEAN_ROUNDS", &in.lean_rounds}});
}
void read_volume_knobs(VolumeIn& in) {
    read_knobs({{"NART_VOL_SPARSE", &in.sparse}, {"NART_VOL_SPARSE_F", &in.sparse_f}, {"NART_VOL_SPARSE_ROUNDS", &in.sparse_rounds}});
}
void read_splat_knobs(SplatIn& in) {
    read_knobs({{"NART_SKEW_BANDS", &in.skew_bands}});
    const char* small = env_opt("NART_SPLAT_SMALL");  // a word, not a number
    in.small_col4 = small && std::strcmp(small, "col4") == 0;
}

// What the scheduling steps of one launch_render share.
using PathKernel = void (*)(DScene, RenderArgs);
struct PathLaunch {
    nart_ctx* ctx;
    hipStream_t st;
    const PathSchedule& plan;
    PathKernel probe;  // k_render with the cost counters, its LDS and its arguments
    size_t lds;
    RenderArgs args;
};

// Cost probe: the first sample of the plan's pixels, work estimates into ctx->d_cost.
int run_probe(const PathLaunch& L) {
    nart_ctx* ctx = L.ctx;
    RenderArgs pb = L.args;
    pb.spp = 1;
    pb.cost = ctx->d_cost.as<uint32_t>();
    pb.probe_sub = L.plan.probe == PathProbe::Sampled ? L.plan.probe_sub : 0u;
    hipLaunchKernelGGL(L.probe, dim3(L.plan.probe_blocks), dim3(256), L.lds, L.st, ctx->scene, pb);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// Groups: the persistent grid's waves take 64-slot groups from b.ghead, in slot order or in b.gorder.
int schedule_groups(const PathLaunch& L, RenderArgs& b) {
    nart_ctx* ctx = L.ctx;
    const QueueBufs q(ctx);
    const PathSchedule& plan = L.plan;
    HIPCHK(hipMemsetAsync(q.qhead, 0, sizeof(uint32_t), L.st));
    b.ghead = q.qhead;
    if (plan.probe == PathProbe::None) return NART_OK;
    const uint32_t ng = (b.n_slots + 63) / 64;
    int rc = run_probe(L);
    if (!rc) rc = sort_groups_by_cost(ctx, b.n_slots, plan.probe_sub, nullptr, L.st);
    if (rc) return rc;
    b.gorder = q.vals[1];
    if (plan.order == 2) {  // the E costliest groups first, each class in slot order
        hipLaunchKernelGGL(k_group_class, dim3((ng + 255) / 256), dim3(256), 0, L.st, q.vals[1], ng, plan.E,
                           q.keys[0], q.vals[0]);
        size_t tmp = q.sort_bytes;
        HIPCHK(hipcub::DeviceRadixSort::SortPairs(q.sort_tmp, tmp, q.keys[0], q.keys[1], q.vals[0],
                                                  q.queue, (int)ng, 0, 1, L.st));
        b.gorder = q.queue;
    }
    return NART_OK;
}

// PixelQueue: the probe-ordered queue (queue_entry) and the refill head of the persistent grid.
// WholeGroupsByCost: one lane per pixel, the groups launched costliest first.
int schedule_pixel_queue(const PathLaunch& L, RenderArgs& b) {
    nart_ctx* ctx = L.ctx;
    const QueueBufs q(ctx);
    const PathSchedule& plan = L.plan;
    const uint32_t n = b.n_slots;
    const bool whole = plan.shape == PathShape::WholeGroupsByCost;
    const dim3 eg((n + 255) / 256), block(256);
    int rc = run_probe(L);
    if (!rc) rc = sort_groups_by_cost(ctx, n, 64, whole ? q.queue : q.cost, L.st);
    b.queue = q.queue;
    if (rc || whole) return rc;
    HIPCHK(hipMemcpyAsync(q.vals[1], q.cost, (size_t)n * 4, hipMemcpyDeviceToDevice, L.st));
    // d_vals[1] = pixels by cost class; partition the rest (slot order) from the top k*W
    hipLaunchKernelGGL(k_flag_top, eg, block, 0, L.st, q.vals[1], n, plan.k * plan.W, q.keys[0]);
    hipLaunchKernelGGL(k_iota, eg, block, 0, L.st, q.cost, n);
    size_t tmp = q.sort_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(q.sort_tmp, tmp, q.keys[0], q.keys[1], q.cost,
                                              q.vals[0], (int)n, 0, 1, L.st));
    hipLaunchKernelGGL(k_build_queue, dim3((plan.qlen + 255) / 256), block, 0, L.st, q.vals[1], q.vals[0], n,
                       plan.W, plan.k, plan.rq_prio ? RQ_PRIO_BIT : 0u, plan.pairs, plan.half, plan.quad, q.queue);
    b.rq_setprio = plan.rq_setprio;
    b.rq_prio = plan.rq_prio;
    b.rq_pairs = plan.pairs;
    b.qlen = plan.qlen;
    HIPCHK(hipMemsetAsync(q.qhead, 0, sizeof(uint32_t), L.st));
    b.qhead = q.qhead;
    b.qbase = plan.qbase;
    return NART_OK;
}

// The camera rays of the batch in `pa` (pa.packet set) into ctx->d_prim.  Packets of one pixel's
// samples (k_primary_px: 4 slots per block, one wave stack each) where the rows are pixel-major, spp
// is a multiple of 64 and packet traversal is on; NART_PRIMARY_PIXEL=0 (a test hook: same hits) and
// every other case: k_primary, a 16x4-pixel block per wave, the per-lane stacks' LDS.
template <bool COUNT, bool ENV, uint32_t FM>
void launch_primary(nart_ctx* ctx, const RenderArgs& pa, hipStream_t st) {
    const bool pixel = pa.packet && ctx->rows_pixel_major && pa.spp % 64u == 0u && env_num("NART_PRIMARY_PIXEL", 1.0) != 0.0;
    if (pixel)
        hipLaunchKernelGGL((k_primary_px<COUNT, ENV, FM>), dim3((pa.n_slots + 3) / 4), dim3(256),
                           (size_t)ctx->stack_depth * 4 * sizeof(uint4), st, ctx->scene, pa, ctx->d_prim.as<uint32_t>());
    else
        hipLaunchKernelGGL((k_primary<COUNT, ENV, FM>), dim3((pa.n_slots + 255) / 256), dim3(256),
                           (size_t)ctx->stack_depth * 256 * 8, st, ctx->scene, pa, ctx->d_prim.as<uint32_t>());
}

// One batch of the path integrator: k_primary, what the plan's shape prepares, the path kernel.
// The template parameters are the kernel builds of `B.id` (dispatch_megakernel's table), `B` their LDS
// layout (host/path_build.h plan_build); host/path_schedule.h plan_path decides the rest.
// resident_k: resident blocks of k_render (dispatch_megakernel's occupancy query).
template <bool EXT, bool COUNT, bool ENV, uint32_t FM = FT_ALL, int WV = 2, bool PR = true, bool LG = false, bool DC = false,
          bool CS = false>
int launch_render(nart_ctx* ctx, const RenderArgs& a_in, const PathBuild& B, uint32_t resident_k, hipStream_t st) {
    auto kern = k_render<EXT, COUNT, ENV>;
    auto kern_rq = k_render_rq<EXT, COUNT, ENV, FM, WV, PR, LG, DC, CS>;
    const uint32_t RQB = B.rq_block;
    RenderArgs a = a_in;
    int rc = EXT ? ensure_ilist(ctx, a) : NART_OK;
    if (rc) return rc;
    static std::atomic<uint64_t> attr{0};  // dynamic LDS above the 64 KiB default, set once per device
    const uint64_t dbit = 1ull << (ctx->device & 63);
    if (!(attr.load() & dbit)) {
        for (const void* f : {(const void*)kern, (const void*)k_render<EXT, true, ENV>,
                              (const void*)kern_rq, (const void*)k_primary<COUNT, ENV, FM>})
            hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr.fetch_or(dbit);
    }
    const bool rq = B.rq;
    ctx->fm_used = B.fm_used;
    RenderArgs b = a;  // k_render's (the cost probe, the fallback), until the ray-queue kernel takes its place
    b.lds_nodes = B.k_render.nodes;
    const size_t lds = B.k_render.bytes, lds_rq = B.rq_lds.bytes;
    uint32_t resident_rq = 1;
    if (rq && (rc = resident_blocks(ctx, (const void*)kern_rq, RQB, lds_rq, &resident_rq))) return rc;

    // (a cost frame leaves the camera rays to the path kernel: k_primary's packets would count a wave's
    // union of steps, not the ray's own)
    const PathLaunchIn in{a.n_slots, resident_k, resident_rq * (RQB / 256), RQB, WV, PR, ENV, rq, FM != FT_ALL,
                          (bool)ctx->d_prim && a.cost == nullptr && !CS};
    const PathSchedule plan = plan_path(in, read_sched_knobs());
    if (plan.error) return fail(ctx, NART_E_INVALID, plan.error);
    ctx->sched |= plan.sched;

    const uint32_t* prim = a.prim;
    if (plan.primary) {
        RenderArgs pa = a;
        pa.packet = plan.packet;
        launch_primary<COUNT, ENV, FM>(ctx, pa, st);
        HIPCHK(hipGetLastError());
        HIPCHK(record(ctx->ev_primary, st));
        ctx->primary_ran = true;
        ctx->prim_valid = true;
        prim = ctx->d_prim.as<uint32_t>();
    }
    if (plan.queue_room && (rc = ensure_queue(ctx, plan.queue_room))) return rc;
    const PathLaunch L{ctx, st, plan, k_render<EXT, true, ENV>, lds, b};
    switch (plan.shape) {
        case PathShape::Direct: break;
        case PathShape::Groups: rc = schedule_groups(L, b); break;
        case PathShape::WholeGroupsByCost:
        case PathShape::PixelQueue: rc = schedule_pixel_queue(L, b); break;
    }
    if (rc) return rc;

    if (!rq) {
        if (LG) return fail(ctx, NART_E_UNSUPPORTED, "light groups need the ray-queue kernel");  // (plan_build refuses it first)
        if (DC) return fail(ctx, NART_E_UNSUPPORTED, "depth cuts need the ray-queue kernel");    // (likewise)
        if (CS) return fail(ctx, NART_E_UNSUPPORTED, "the cost image needs the ray-queue kernel");  // (likewise)
        hipLaunchKernelGGL(kern, dim3(plan.blocks), dim3(256), lds, st, ctx->scene, b);
        HIPCHK(hipGetLastError());
        return NART_OK;
    }
    // the ray-queue kernel takes k_render's place, with its own LDS layout
    b.lds_nodes = B.rq_lds.nodes;
    b.prim = prim;
    b.stack_lds = B.stack_lds;
    b.rq_quorum = plan.rq_quorum;
    const uint32_t per = RQB / 256;  // the plan counts launches in blocks of 256
    const uint32_t grid = (plan.blocks + per - 1) / per;
    const size_t threads = (size_t)grid * RQB;
    // per-thread global columns, indexed by the global thread id: sized from this grid
    if (EXT && threads > b.ilist_stride) return fail(ctx, NART_E_INVALID, "dielectric-list columns smaller than the launch");
    if (B.stack_lds < ctx->stack_depth && (rc = ensure_gstack(ctx, threads, ctx->stack_depth - B.stack_lds, b))) return rc;
    hipLaunchKernelGGL(kern_rq, dim3(grid), dim3(RQB), lds_rq, st, ctx->scene, b);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// One instantiation of launch_render per build of the path kernels that plan_build can name.
using RenderLauncher = int (*)(nart_ctx*, const RenderArgs&, const PathBuild&, uint32_t, hipStream_t);
struct BuildRow {
    BuildId id;
    RenderLauncher launch;
};
template <bool EXT, bool COUNT, bool ENV, uint32_t FM = FT_ALL, int WV = 2, bool PR = true, bool LG = false, bool DC = false,
          bool CS = false>
BuildRow build_row() {
    return {BuildId{EXT, COUNT, ENV, FM, WV, PR, LG, DC, CS}, launch_render<EXT, COUNT, ENV, FM, WV, PR, LG, DC, CS>};
}

int dispatch_megakernel(nart_ctx* ctx, const RenderArgs& a, hipStream_t st) {
    PathBuildIn in;
    in.features = ctx->features;
    in.has_env = ctx->has_env;
    in.specialize = !ctx->specialize ? Specialize::Off : (ctx->lean ? Specialize::Lean : Specialize::On);
    in.counters = ctx->counters;
    in.depth_cuts = a.n_groups != 0 && a.cuts[0] != 0;  // (the record arrays are the cuts' where cuts are given)
    in.light_groups = a.n_groups != 0 && !in.depth_cuts;
    in.cost = a.cost_rec != nullptr;
    in.bounces = a.bounces;
    in.variant = ctx->variant;
    in.stack_depth = ctx->stack_depth;
    in.num_nodes = ctx->num_nodes;
    in.n_slots = a.n_slots;
    // resident blocks of k_render, the figure every threshold in rounds of resident waves refers to
    // (plan_build, plan_path).  Every k_render build is compiled for two waves per SIMD and has the
    // same LDS, so one build's occupancy stands for all of them.
    int rc = resident_blocks(ctx, (const void*)k_render<false, false, false>, 256,
                             k_render_layout(ctx->stack_depth, ctx->num_nodes).bytes, &in.resident_k);
    if (rc) return rc;
    read_build_knobs(in);
    const PathBuild B = plan_build(in);
    if (B.error) return fail(ctx, B.unsupported ? NART_E_UNSUPPORTED : NART_E_INVALID, B.error);
    // every build plan_build can name (tests/test_path_build.py, test_path_build_lights.py,
    // test_path_build_depth.py and test_path_build_cost.py hold the same list; new rows go at the end).  The compiler emits
    // the kernels in the order of the rows: keep it, and the gfx950 code object stays byte for byte the same
    static const BuildRow builds[] = {
        build_row<false, false, false, FM_DIFFUSE, 3, false>(),  // scene-specialised: lean, two waves per SIMD
        build_row<false, false, false, FM_DIFFUSE>(),
        build_row<false, false, false, FM_GLASS, 3, false>(),
        build_row<false, false, false, FM_GLASS>(),
        build_row<false, false, true, FM_ENVTEX, 3, false>(),
        build_row<false, false, true, FM_ENVTEX>(),
        build_row<false, true, true>(),  // generic: EXT x COUNT x ENV
        build_row<false, false, true>(),
        build_row<true, true, true>(),
        build_row<true, false, true>(),
        build_row<false, true, false>(),
        build_row<false, false, false>(),
        build_row<true, true, false>(),
        build_row<true, false, false>(),
        build_row<false, false, true, FT_ALL, 2, false, true>(),  // light groups: EXT x ENV
        build_row<true, false, true, FT_ALL, 2, false, true>(),
        build_row<false, false, false, FT_ALL, 2, false, true>(),
        build_row<true, false, false, FT_ALL, 2, false, true>(),
        build_row<false, false, true, FT_ALL, 2, false, false, true>(),  // depth cuts: EXT x ENV
        build_row<true, false, true, FT_ALL, 2, false, false, true>(),
        build_row<false, false, false, FT_ALL, 2, false, false, true>(),
        build_row<true, false, false, FT_ALL, 2, false, false, true>(),
        build_row<false, false, true, FT_ALL, 2, false, false, false, true>(),  // cost image: EXT x ENV
        build_row<true, false, true, FT_ALL, 2, false, false, false, true>(),
        build_row<false, false, false, FT_ALL, 2, false, false, false, true>(),
        build_row<true, false, false, FT_ALL, 2, false, false, false, true>(),
    };
    for (const BuildRow& row : builds)
        if (row.id == B.id) return row.launch(ctx, a, B, in.resident_k, st);
    return fail(ctx, NART_E_INVALID, "no path-kernel build for the plan");
}

// Volume integrator (k_render_volume_sm): host/path_schedule.h plan_volume and sparse_hot_groups decide
// the launch, this executes it.
int dispatch_volume(nart_ctx* ctx, const RenderArgs& a, hipStream_t st) {
    const dim3 block(256);
    const uint32_t n = a.n_slots;
    VolumeIn in;
    in.n_slots = n;
    in.spp = a.spp;
    in.grid_cells = ctx->scene.medium.present ? ctx->scene.medium.rx * ctx->scene.medium.ry * ctx->scene.medium.rz : 0;
    in.counters = ctx->counters;
    const size_t dl = (size_t)volume_lds_cells(in.grid_cells) * sizeof(float);
    int rc = resident_blocks(ctx, (const void*)k_render_volume_sm<false, 1>, 256, dl, &in.resident);
    if (rc) return rc;
    read_volume_knobs(in);
    const VolumePlan plan = plan_volume(in);
    RenderArgs b = a;
    b.lds_nodes = plan.lds_nodes;
    uint32_t grid = plan.blocks;
    ctx->sched |= plan.sched;
    if (plan.queue) {
        if ((rc = ensure_queue(ctx, plan.queue_room))) return rc;
        const QueueBufs q(ctx);
        RenderArgs pb = b;
        pb.spp = 4;
        pb.cost = q.cost;
        hipLaunchKernelGGL((k_render_volume_sm<false, 1>), dim3(plan.blocks), block, dl, st, ctx->scene, pb);
        rc = sort_groups_by_cost(ctx, n, 64, q.queue, st);
        if (rc) return rc;
        b.queue = q.queue;
        if (plan.sparse) {
            const uint32_t ng = (n + 63) / 64;
            std::vector<uint32_t> keys(ng);
            HIPCHK(hipMemcpyAsync(keys.data(), q.keys[1], (size_t)ng * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const SparseGroups hot = sparse_hot_groups(keys.data(), ng, plan.f, plan.S, plan.W, n);
            if (hot.H) {
                hipLaunchKernelGGL(k_sparse_groups, dim3(hot.grid), block, 0, st, q.vals[1], n, hot.H, plan.S,
                                   hot.qlen, q.queue);
                b.qlen = hot.qlen;
                grid = hot.grid;
                ctx->sched |= NART_SCHED_VOL_SPARSE;
            }
        }
        HIPCHK(hipGetLastError());
    }
    switch (plan.build) {
        case VolumeBuild::Counter: hipLaunchKernelGGL((k_render_volume_sm<true, 1>), dim3(grid), block, dl, st, ctx->scene, b); break;
        case VolumeBuild::FourWave: hipLaunchKernelGGL((k_render_volume_sm<false, NART_VOL_WV>), dim3(grid), block, dl, st, ctx->scene, b); break;
        case VolumeBuild::Plain: hipLaunchKernelGGL((k_render_volume_sm<false, 1>), dim3(grid), block, dl, st, ctx->scene, b); break;
    }
    HIPCHK(hipGetLastError());
    return NART_OK;
}

int dispatch_render(nart_ctx* ctx, const RenderArgs& a, int integrator, hipStream_t st) {
    if (integrator == NART_INTEGRATOR_VOLUME) return dispatch_volume(ctx, a, st);
    return dispatch_megakernel(ctx, a, st);
}

// LatinSquare samples of the batch in `ra`, in the form and launch shapes of host/latin_plan.h plan_latin;
// the three-kernel form's scratch arrays lie in ra.Lout, which the path kernel overwrites later.
int launch_latin(nart_ctx* ctx, const RenderArgs& ra, hipStream_t st) {
    const LatinPlan lp = plan_latin(ra.n_slots, ra.spp, ctx->cap_samples * sizeof(float4));
    auto launch = [&](auto kernel, const Grid& g, auto... args) {
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(g.threads), g.lds, st, ra, args...);
    };
    switch (lp.form) {
    case LatinForm::Three: {
        uint32_t* const base = reinterpret_cast<uint32_t*>(ra.Lout);
        const LatinScratch ls{base + lp.cx, base + lp.cy, base + lp.sx, base + lp.sy, base + lp.st, lp.n2};
        launch(k_latin_draws, lp.draws, ls);
        if (lp.perm_block == 80) launch(k_latin_perm<80>, lp.perm, ls);
        else launch(k_latin_perm<64>, lp.perm, ls);
        launch(k_latin_emit, lp.emit, ls);
        break;
    }
    case LatinForm::Lds: launch(k_latin_lds, lp.one); break;
    case LatinForm::Idx: launch(k_latin_idx, lp.one, (float*)ra.Lout); break;
    case LatinForm::Global: launch(k_latin, lp.one); break;
    }
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// ---------------------------------------------------------------- first-hit AOVs
// A plan (host/frame_plan.h) with its outputs' tile buffers: tiles[i] receives the splatted records of
// plan.outputs[i], laid out like the beauty tiles, in the order of the bucket list rendered.
static_assert(FRAME_MAX_LAYERS == CASCADE_MAX_LAYERS && FRAME_MAX_PLANES == MATTE_MAX_PLANES &&
                  FRAME_MAX_MATTE_IDS == MATTE_MAX_IDS && FRAME_MAX_LIGHT_GROUPS == LIGHT_GROUPS_MAX &&
                  FRAME_MAX_LIGHT_GROUPS == NART_LIGHT_GROUPS_MAX && FRAME_MAX_DEPTH_CUTS == DEPTH_CUTS_MAX &&
                  FRAME_MAX_DEPTH_CUTS == NART_DEPTH_CUTS_MAX && sizeof(RenderArgs::cuts) == 4 * DEPTH_CUTS_MAX,
              "frame_plan.h restates the device headers' limits");
struct FrameTiles {
    FramePlan plan;
    float* tiles[FRAME_MAX_OUTPUTS] = {};

    // the outputs' buffers back to back from `base`, `slab` floats each
    FrameTiles(const FramePlan& pl, float* base, size_t slab) : plan(pl) {
        for (uint32_t i = 0; i < plan.n_outputs; ++i) tiles[i] = base + i * slab;
    }
    float* of(OutputKind kind) const {
        const int i = plan.find(kind);
        return i < 0 ? nullptr : tiles[i];
    }
};
// Device time of each pass of a render (frame_plan.h PassKind), added up over its batches.
struct PassTimes {
    double ms[PASS_SLOTS] = {};
};

// Camera-ray hits of the batch in `a` into ctx->d_prim, for AOVs of a dispatch that did not run
// k_primary itself (variant 3, the LDS fallback, an AOV-only render): the generic build, launched
// as launch_render launches it.
int launch_aov_primary(nart_ctx* ctx, const RenderArgs& a, hipStream_t st) {
    RenderArgs pa = a;
    pa.packet = env_num("NART_PRIMARY_PACKET", 1.0) != 0.0 ? 1u : 0u;
    const void* f = ctx->has_env ? (const void*)k_primary<false, true, FT_ALL> : (const void*)k_primary<false, false, FT_ALL>;
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    if (ctx->has_env) launch_primary<false, true, FT_ALL>(ctx, pa, st);
    else launch_primary<false, false, FT_ALL>(ctx, pa, st);
    HIPCHK(hipGetLastError());
    ctx->prim_valid = true;
    return NART_OK;
}

// Per-sample records of AOV `rec` of the batch in `a` (ctx->d_prim valid) into `out`.
int launch_aov(nart_ctx* ctx, const RenderArgs& a, int rec, float4* out, hipStream_t st) {
    const dim3 grid((a.n_slots + 255) / 256), block(256);
    const uint32_t* hits = ctx->d_prim.as<uint32_t>();
    if (rec == AOV_ALBEDO) hipLaunchKernelGGL((k_aov<AOV_ALBEDO>), grid, block, 0, st, ctx->scene, a, hits, out);
    else hipLaunchKernelGGL((k_aov<AOV_NORMAL>), grid, block, 0, st, ctx->scene, a, hits, out);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// The followed-guide chains of the batch in `a` (device/guide.h k_guide): ga.albedo and ga.normal
// receive the records, either may be null.  Launched as the per-lane k_primary: 256-lane blocks on
// stack_depth * 256 * 8 bytes of LDS.
template <bool DUMP>
int launch_guide(nart_ctx* ctx, const RenderArgs& a, const GuideArgs& ga, hipStream_t st) {
    const void* f = ctx->has_env ? (const void*)k_guide<true, DUMP> : (const void*)k_guide<false, DUMP>;
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const dim3 grid((a.n_slots + 255) / 256), block(256);
    const size_t lds = (size_t)ctx->stack_depth * 256 * 8;
    if (ctx->has_env) hipLaunchKernelGGL((k_guide<true, DUMP>), grid, block, lds, st, ctx->scene, a, ga);
    else hipLaunchKernelGGL((k_guide<false, DUMP>), grid, block, lds, st, ctx->scene, a, ga);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// s into `into`, field by field (render_ms is the caller's wall clock: RenderTimer).  Device times
// and the launch count add up over the batches and renders of one device (Sum) and take the slowest
// of devices that run concurrently (Max); work counts always add up.
enum class Times { Sum, Max };
void add_stats(nart_render_stats& into, const nart_render_stats& s, Times how) {
    auto time = [how](auto& a, auto b) { a = how == Times::Max ? std::max(a, b) : a + b; };
    time(into.kernel_ms, s.kernel_ms);
    time(into.splat_ms, s.splat_ms);
    time(into.latin_ms, s.latin_ms);
    time(into.primary_ms, s.primary_ms);
    time(into.kernel_launches, s.kernel_launches);
    into.schedule |= s.schedule;
    into.samples += s.samples;
    into.traced_samples += s.traced_samples;
    into.rays_extend += s.rays_extend;
    into.rays_shadow += s.rays_shadow;
    into.node_visits += s.node_visits;
    into.tri_tests += s.tri_tests;
    into.bounces += s.bounces;
    into.octree_checks += s.octree_checks;
    into.octree_replays += s.octree_replays;
}

// Wall time of a scope into stats->render_ms (a call that fails adds the time it took, too).
struct RenderTimer {
    nart_render_stats* stats;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit RenderTimer(nart_render_stats* s) : stats(s) {}
    RenderTimer(const RenderTimer&) = delete;
    ~RenderTimer() {
        using ms = std::chrono::duration<double, std::milli>;
        if (stats) stats->render_ms += ms(std::chrono::steady_clock::now() - t0).count();
    }
};

// Kernel arguments of n_slots slots laid out in the context's work buffers (ensure).
RenderArgs make_render_args(const nart_ctx* ctx, const nart_render_params* p, const nart_session_geometry& g,
                            uint32_t n_slots, unsigned long long* counters) {
    RenderArgs ra;
    ra.slot_xy = ctx->d_slot_xy.as<uint32_t>();
    ra.slot_so = ctx->d_slot_so.as<SlotSO>();
    ra.samples = ctx->d_samples.as<float2>();
    ra.rng0 = ctx->d_rng.as<uint32_t>();
    ra.Lout = ctx->d_L.as<float4>();
    ra.n_slots = n_slots;
    ra.spp = p->spp;
    ra.bounces = p->bounces;
    ra.W = p->image_width;
    ra.H = p->image_height;
    ra.totalW = g.total_width;
    ra.stack_depth = ctx->stack_depth;
    ra.lds_nodes = 0;
    ra.gamma = p->roughening_factor * p->roughening_factor;
    ra.counters = counters;
    return ra;
}

// How a render_buckets call splats: the kernel and sample layout (host/splat_plan.h plan_splat), and the
// SplatArgs fields that hold for the whole call (the batch adds its buckets, samples and tiles).
static_assert(sizeof(LutCell) == sizeof(float4), "the splat kernels read the filter cells as float4");
struct SplatPlan {
    SplatArgs sa;
    SplatChoice choice;
};

// The splat of a call over n_buckets buckets; uploads the filter table, thresholds and LUT.
int plan_splat(nart_ctx* ctx, const nart_render_params* p, const nart_session_geometry& g, uint32_t n_buckets,
               SplatPlan& plan) {
    // filter table [64] + filter-index thresholds [65] (splat_thresholds)
    float table[64 + 65];
    nart_filter_table(table);
    const bool thr_ok = splat_thresholds(p->filter_width, table + 64);
    if (int rc = reserve(ctx, ctx->d_table, ctx->device, sizeof(table), "filter table")) return rc;
    float* const d_table = ctx->d_table.as<float>();
    HIPCHK(hipMemcpy(d_table, table, sizeof(table), hipMemcpyHostToDevice));
    std::vector<LutCell> lut;
    uint32_t lut_b0 = 0;
    const bool lut_ok = thr_ok && splat_lut(table + 64, table, lut, lut_b0);
    if (lut_ok) {
        if (int rc = reserve(ctx, ctx->d_lut, ctx->device, SPLAT_LUT_MAX * sizeof(float4), "splat filter cells")) return rc;
        HIPCHK(hipMemcpy(ctx->d_lut.as<float4>(), lut.data(), lut.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
    int n_cus = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
    SplatIn in;
    in.mode = ctx->splat_mode;
    in.volume = p->integrator == NART_INTEGRATOR_VOLUME;
    in.B = p->bucket_size;
    in.fb = g.filter_bounds;
    in.tile = p->bucket_size + 2 * g.filter_bounds;
    in.n_buckets = n_buckets;
    in.n_cus = (uint32_t)n_cus;
    in.lut_ok = lut_ok;
    read_splat_knobs(in);
    plan.choice = plan_splat(in);
    const SplatScalars v = splat_scalars(p->filter_width, p->spp, p->bucket_size, g.filter_bounds, g.tile_size, g.n_buckets_x,
                                         g.total_width, g.total_height, lut_b0, (uint32_t)lut.size());
    SplatArgs& sa = plan.sa;
    sa.table = d_table;
    sa.thr = thr_ok ? d_table + 64 : nullptr;
    sa.lut = lut_ok ? ctx->d_lut.as<const float4>() : nullptr;
    sa.idx_scale = v.idx_scale;
    sa.spp = v.spp, sa.B = v.B, sa.fb = v.fb, sa.tile = v.tile, sa.nbx = v.nbx, sa.totalW = v.totalW, sa.totalH = v.totalH;
    sa.fw = v.fw, sa.invB = v.invB, sa.invFw = v.invFw;
    sa.lut_b0 = v.lut_b0, sa.lut_n = v.lut_n;
    return NART_OK;
}

// sa.Lout into sa.tiles for the nbk buckets of a batch: the beauty, then each requested AOV's
// records, by the same kernel, launched as host/splat_plan.h splat_launch says.
// MOM: the moment image's pass (kernels.h k_moment): the same kernel and launch shape.
template <bool MOM>
int launch_splat_as(nart_ctx* ctx, const SplatPlan& plan, const SplatArgs& sa, uint32_t nbk, hipStream_t st) {
    const SplatLaunch l = splat_launch(plan.choice, sa.fb, sa.tile, sa.thr != nullptr, sa.invB != 0.f, sa.lut ? sa.lut_n : 0u, nbk);
    using Kernel = void (*)(SplatArgs);
    Kernel k = nullptr;
    switch (l.kernel) {
    case SplatKernel::Rows: {
        static const Kernel rows[3] = {k_splat_rows<1, MOM>, k_splat_rows<2, MOM>, k_splat_rows<3, MOM>};
        k = rows[l.fb - 1];
        break;
    }
    case SplatKernel::Skew: {
        static const Kernel skew[3][2] = {{k_splat_skew<1, 1, MOM>, k_splat_skew<1, 2, MOM>},
                                          {k_splat_skew<2, 1, MOM>, k_splat_skew<2, 2, MOM>},
                                          {k_splat_skew<3, 1, MOM>, k_splat_skew<3, 2, MOM>}};
        k = skew[l.fb - 1][l.bands - 1];
        break;
    }
    case SplatKernel::Col4: k = l.lut ? k_splat_col4<NART_SPLAT_NP, true, MOM> : k_splat_col4<NART_SPLAT_NP, false, MOM>; break;
    case SplatKernel::Pixel: k = l.thr ? k_splat<1, MOM> : k_splat<0, MOM>; break;
    }
    ctx->sched |= l.sched;
    hipLaunchKernelGGL(k, dim3(l.blocks), dim3(l.threads), l.lds, st, sa);
    HIPCHK(hipGetLastError());
    return NART_OK;
}
int launch_splat(nart_ctx* ctx, const SplatPlan& plan, const SplatArgs& sa, uint32_t nbk, hipStream_t st,
                 bool moment = false) {
    return moment ? launch_splat_as<true>(ctx, plan, sa, nbk, st) : launch_splat_as<false>(ctx, plan, sa, nbk, st);
}

// The per-sample records of output `w` for the ns samples of the nbk buckets of the batch in `ra`, which the splat then takes
// into the output's tiles: one small kernel fills `records` from the beauty's records (ctx->d_L) or the
// camera-ray hits (ctx->d_prim).  The guides' records were filled at the start of their pass (`ga`).
// Returns the records to splat.
int fill_records(nart_ctx* ctx, const FramePlan& frame, const FrameOutput& w, const RenderArgs& ra, const GuideArgs& ga,
                 float4* records, uint64_t ns, uint32_t nbk, hipStream_t st, const float4** filled) {
    const dim3 grid((uint32_t)((ns + 255) / 256)), block(256);
    *filled = records;
    switch (w.kind) {
    case OutputKind::Layer: {
        const CascadeLevels& lv = frame.ask.cascade;
        CascadeSplitArgs ca;
        ca.L = ctx->d_L.as<float4>();
        ca.out = records;
        ca.n = ns;
        ca.K = lv.K;
        ca.b_first = lv.b[0];
        ca.b_top = lv.b[lv.K - 1];
        ca.base_m1 = lv.base - 1.f;
        ca.j = w.index;
        ca.b_prev = ca.j > 0 ? lv.b[ca.j - 1] : 0.f;
        ca.b_cur = lv.b[ca.j];
        ca.b_next = ca.j + 1 < lv.K ? lv.b[ca.j + 1] : 0.f;
        hipLaunchKernelGGL(k_cascade_split, grid, block, 0, st, ca);
        break;
    }
    case OutputKind::HalfA:
    case OutputKind::HalfB: {
        HalfSplitArgs ha;
        ha.L = ctx->d_L.as<float4>();
        ha.out = records;
        ha.n = ns;
        ha.bucket_base = ctx->d_bucket_base.as<uint32_t>();
        ha.nbk = nbk;
        ha.n_slots = ra.n_slots;
        ha.spp = ra.spp;
        ha.h = w.kind == OutputKind::HalfA ? 0u : 1u;
        ha.pixel_major = ctx->rows_pixel_major ? 1u : 0u;
        hipLaunchKernelGGL(k_half_split, grid, block, 0, st, ha);
        break;
    }
    case OutputKind::Moment: hipLaunchKernelGGL(k_moment, grid, block, 0, st, ctx->d_L.as<float4>(), ns); break;
    case OutputKind::Albedo:
    case OutputKind::Normal:
        if (int rc = launch_aov(ctx, ra, w.kind == OutputKind::Albedo ? AOV_ALBEDO : AOV_NORMAL, records, st)) return rc;
        break;
    case OutputKind::Plane: {
        MatteIdArgs ma;
        ma.hit = ctx->d_prim.as<uint32_t>();
        ma.tri_mesh = ctx->scene.tri_mesh;
        ma.meshes = ctx->scene.meshes;
        ma.out = ctx->d_L.as<float4>();
        ma.n = ns;
        ma.num_tris = ctx->scene.num_tris;
        ma.num_meshes = ctx->num_meshes;
        ma.kind = frame.ask.matte.kind;
        ma.n_ids = frame.ask.matte.n_ids;
        ma.q = w.index;
        hipLaunchKernelGGL(k_matte_ids, grid, block, 0, st, ma);
        break;
    }
    case OutputKind::GuideAlbedo: *filled = ga.albedo; break;
    case OutputKind::GuideNormal: *filled = ga.normal; break;
    case OutputKind::Beauty:
    case OutputKind::LightGroup:
    case OutputKind::DepthCut: break;  // (no pass: pass_of)
    }
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// The device times of a batch from its event pairs, once the last event recorded has been waited for:
// the passes' into `times`, the light groups' or depth cuts' splats into group_ms, the rest into acc.
int read_batch_times(nart_ctx* ctx, const FramePlan& frame, bool groups, nart_render_stats& acc, PassTimes* times,
                     double& group_ms) {
    float ms = 0.f;
    for (uint32_t i = 0; i < frame.n_passes && times; ++i) {
        const PassKind pass = frame.passes[i];
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev_pass[pass][0].handle(), ctx->ev_pass[pass][1].handle()));
        times->ms[pass] += ms;
    }
    if (groups) {
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev_lg[0].handle(), ctx->ev_lg[1].handle()));
        group_ms += ms;
    }
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_path0.handle(), ctx->ev_path1.handle()));
    acc.kernel_ms += ms;
    if (ctx->primary_ran) {
        HIPCHK(hipEventElapsedTime(&ms, ctx->ev_path0.handle(), ctx->ev_primary.handle()));
        acc.primary_ms += ms;
    }
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_path1.handle(), ctx->ev_splat1.handle()));
    acc.splat_ms += ms;
    HIPCHK(hipEventElapsedTime(&ms, ctx->ev_latin0.handle(), ctx->ev_path0.handle()));
    acc.latin_ms += ms;
    return NART_OK;
}

// Render a bucket list into device tiles (list order); p is validated by the caller (check_params).
// Shared by all entry points.  After the path kernel and the beauty's splat each batch runs the
// frame plan's passes (frame_plan.h PassKind, which gives their order and why): per output of the pass, one
// small kernel fills a record buffer (fill_records) -- ctx->d_L, which the beauty splat has consumed by
// then, so no extra per-sample memory; for the cascade a second record buffer, a temporary of this call --
// and the same splat kernel takes it into that output's tiles.  The guide pass fills the records of both its
// outputs by one k_guide launch at its start (the normal record in a temporary of this call where
// both are asked for).  times: the passes' device times are added.
int render_buckets(nart_ctx* ctx, const nart_render_params* p, const uint32_t* ids, uint32_t n, const FrameTiles& out,
                   hipStream_t st, nart_render_stats* stats, PassTimes* times = nullptr) {
    int rc = NART_OK;
    const FramePlan& frame = out.plan;
    const bool beauty = frame.path_kernel;
    HIPCHK(hipSetDevice(ctx->device));
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    const uint32_t nb_total = g.n_buckets_x * g.n_buckets_y;
    for (uint32_t i = 0; i < n; ++i)
        if (ids[i] >= nb_total) return fail(ctx, NART_E_INVALID, "bucket id out of range");
    SplatPlan plan;
    if ((rc = plan_splat(ctx, p, g, n, plan))) return rc;
    if ((rc = counter_buffer(ctx))) return rc;
    unsigned long long* const d_counters = ctx->d_counters.as<unsigned long long>();
    if (ctx->counters) HIPCHK(hipMemsetAsync(d_counters, 0, ctx->d_counters.bytes(), st));
    const size_t limit = batch_slot_limit(ctx, p->spp, frame.record_bytes);
    Buf layer_records;  // cascade, halves: the second per-sample record buffer, 16 B per sample; freed on return
    Buf guide_records;  // both followed guides: the normal records, likewise (a halves frame: in layer_records,
                        // which its first pass has left free)
    Buf group_records;  // light groups or depth cuts: R record arrays of the batch's samples, likewise
    const uint32_t G = beauty ? frame.ask.light_groups : 0u;
    if (G && !ctx->d_light_group) return fail(ctx, NART_E_INVALID, "no light-group map was set");
    // depth cuts: the K cuts of the call (set_depth_cuts); they share the groups' arrays, splats and events
    const uint32_t K = beauty && !G ? frame.ask.depth_cuts : 0u;
    if (K && ctx->n_depth_cuts != K) return fail(ctx, NART_E_INVALID, "no depth cuts were set");
    const uint32_t R = G ? G : K;
    // cost image: the batch's cost records, and the grid of this device they are reduced into
    Buf cost_records;  // one uint4 per sample of the batch; freed on return
    const bool CS = beauty && frame.ask.cost;
    if (CS && (!ctx->d_cost_grid || ctx->d_cost_grid.bytes() < (size_t)ctx->cost_grid_w * ctx->cost_grid_h * sizeof(uint4) ||
               ctx->cost_grid_w != std::min(p->bucket_size * g.n_buckets_x, g.total_width) ||
               ctx->cost_grid_h != std::min(p->bucket_size * g.n_buckets_y, g.total_height)))
        return fail(ctx, NART_E_INVALID, "no cost grid was set");
    double cost_ms = 0.0;
    double group_ms = 0.0;
    const uint32_t tpx = g.tile_size * g.tile_size;
    const BucketGrid grid{p->bucket_size, g.n_buckets_x, g.total_width, g.total_height, p->image_width, p->image_height};
    nart_render_stats acc;  // this call's share, added to *stats at the end
    std::memset(&acc, 0, sizeof(acc));
    uint64_t counted = 0;
    ctx->sched = 0;
    std::vector<uint32_t> xy, base;
    for (uint32_t b0 = 0, b1; b0 < n; b0 = b1) {
        // gather a batch of buckets whose traced pixels fit the slot budget, and upload it
        b1 = gather_batch(grid, ids, b0, n, limit, xy, base, counted);
        const uint32_t nslots = (uint32_t)xy.size(), nbk = b1 - b0;
        const uint64_t ns = (uint64_t)nslots * p->spp;
        acc.traced_samples += ns;
        rc = ensure(ctx, nslots, p->spp, nbk);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->d_slot_xy.as<uint32_t>(), xy.data(), (size_t)nslots * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_bucket_ids.as<uint32_t>(), ids + b0, (size_t)nbk * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->d_bucket_base.as<uint32_t>(), base.data(), (size_t)nbk * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_slot_table, dim3(nbk), dim3(256), 0, st, ctx->d_bucket_base.as<uint32_t>(), nbk, nslots, p->spp,
                           ctx->d_slot_so.as<SlotSO>(), plan.choice.skew);
        ctx->rows_pixel_major = plan.choice.skew;
        RenderArgs ra = make_render_args(ctx, p, g, nslots, d_counters);
        if (R) {
            if ((rc = reserve(ctx, group_records, ctx->device, (size_t)R * ns * sizeof(float4),
                              G ? "light-group records" : "depth-cut records")))
                return rc;
            ra.n_groups = R;
            ra.Lgrp = group_records.as<float4>();
            ra.lgrp_stride = ns;
        }
        if (G) {
            // the group records start at +0: every sample's owner lane accumulates into them
            HIPCHK(hipMemsetAsync(group_records.as<void>(), 0, (size_t)G * ns * sizeof(float4), st));
            ra.light_group = ctx->d_light_group.as<uint32_t>();
        }
        // (the cut records need no memset: the owner lane writes every one in full)
        for (uint32_t j = 0; j < K; ++j) ra.cuts[j] = ctx->depth_cuts[j];
        if (CS) {
            // (no memset: the owner lane writes every record in full)
            if ((rc = reserve(ctx, cost_records, ctx->device, ns * sizeof(uint4), "cost records"))) return rc;
            ra.cost_rec = cost_records.as<uint4>();
        }
        // LatinSquare, path kernel, the beauty's splat
        HIPCHK(record(ctx->ev_latin0, st));
        rc = launch_latin(ctx, ra, st);
        if (rc) return rc;
        HIPCHK(record(ctx->ev_path0, st));
        ctx->primary_ran = false;
        ctx->prim_valid = false;
        if (beauty) {
            rc = dispatch_render(ctx, ra, p->integrator, st);
            if (rc) return rc;
        }
        HIPCHK(record(ctx->ev_path1, st));
        SplatArgs sa = plan.sa;
        sa.bucket_ids = ctx->d_bucket_ids.as<uint32_t>();
        sa.bucket_base = ctx->d_bucket_base.as<uint32_t>();
        sa.samples = ctx->d_samples.as<float2>();
        sa.Lout = ctx->d_L.as<float4>();
        sa.tiles = beauty ? out.of(OutputKind::Beauty) + (size_t)b0 * tpx * 5 : nullptr;
        sa.n_buckets = nbk;
        if (beauty && (rc = launch_splat(ctx, plan, sa, nbk, st))) return rc;
        HIPCHK(record(ctx->ev_splat1, st));
        hipEvent_t last = ctx->ev_splat1.handle();
        if (R) {
            // the path kernel's own group or cut records, each into its output's tiles by the beauty's splat
            HIPCHK(record(ctx->ev_lg[0], st));
            for (uint32_t o = 0; o < frame.n_outputs; ++o) {
                const FrameOutput& w = frame.outputs[o];
                if (w.kind != (G ? OutputKind::LightGroup : OutputKind::DepthCut)) continue;
                sa.Lout = group_records.as<float4>() + (size_t)w.index * ns;
                sa.tiles = out.tiles[o] + (size_t)b0 * tpx * 5;
                if ((rc = launch_splat(ctx, plan, sa, nbk, st))) return rc;
            }
            HIPCHK(record(ctx->ev_lg[1], st));
            last = ctx->ev_lg[1].handle();
        }
        if (CS) {
            // the batch's cost records summed per slot into the grid (every pixel belongs to one batch)
            CostReduceArgs ca;
            ca.records = cost_records.as<uint4>();
            ca.slot_xy = ctx->d_slot_xy.as<uint32_t>();
            ca.slot_so = ctx->d_slot_so.as<SlotSO>();
            ca.grid = ctx->d_cost_grid.as<uint4>();
            ca.n_slots = nslots;
            ca.spp = p->spp;
            ca.grid_w = ctx->cost_grid_w;
            ca.grid_h = ctx->cost_grid_h;
            HIPCHK(record(ctx->ev_cost[0], st));
            hipLaunchKernelGGL(k_cost_reduce, dim3((nslots + 255) / 256), dim3(256), 0, st, ca);
            HIPCHK(hipGetLastError());
            HIPCHK(record(ctx->ev_cost[1], st));
            last = ctx->ev_cost[1].handle();
        }
        // the frame plan's passes
        for (uint32_t i = 0; i < frame.n_passes; ++i) {
            const PassKind pass = frame.passes[i];
            if ((pass == PASS_CASCADE || pass == PASS_HALVES) &&
                (rc = reserve(ctx, layer_records, ctx->device, ns * sizeof(float4),
                              pass == PASS_CASCADE ? "cascade layer records" : "half-buffer records")))
                return rc;
            // the dispatch's own camera-ray hits where it traced them first, else k_primary now
            if ((pass == PASS_FIRST_HIT || pass == PASS_MATTE) && !ctx->prim_valid && (rc = launch_aov_primary(ctx, ra, st)))
                return rc;
            const bool two_guides = pass == PASS_GUIDE && frame.ask.guide[0] && frame.ask.guide[1];
            Buf& normal_records = frame.ask.halves ? layer_records : guide_records;
            if (two_guides && (rc = reserve(ctx, normal_records, ctx->device, ns * sizeof(float4), "guide normal records")))
                return rc;
            HIPCHK(record(ctx->ev_pass[pass][0], st));
            float4* const records = (pass == PASS_CASCADE || pass == PASS_HALVES ? layer_records : ctx->d_L).as<float4>();
            GuideArgs ga;
            if (pass == PASS_GUIDE) {
                ga.max_follow = frame.ask.max_follow;
                if (frame.ask.guide[0]) ga.albedo = records;
                if (frame.ask.guide[1]) ga.normal = two_guides ? normal_records.as<float4>() : records;
                if ((rc = launch_guide<false>(ctx, ra, ga, st))) return rc;
            }
            for (uint32_t o = 0; o < frame.n_outputs; ++o) {
                const FrameOutput& w = frame.outputs[o];
                if (pass_of(w.kind) != pass) continue;
                if ((rc = fill_records(ctx, frame, w, ra, ga, records, ns, nbk, st, &sa.Lout))) return rc;
                sa.tiles = out.tiles[o] + (size_t)b0 * tpx * 5;
                if ((rc = launch_splat(ctx, plan, sa, nbk, st, pass == PASS_MOMENT))) return rc;
            }
            HIPCHK(record(ctx->ev_pass[pass][1], st));
            last = ctx->ev_pass[pass][1].handle();
        }
        // one stream: waiting for the last event recorded is waiting for all of them
        HIPCHK(hipEventSynchronize(last));
        if ((rc = read_batch_times(ctx, frame, R != 0, acc, times, group_ms))) return rc;
        if (CS) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ctx->ev_cost[0].handle(), ctx->ev_cost[1].handle()));
            cost_ms += ms;
        }
        if (beauty) ++acc.kernel_launches;
    }
    if (G) ctx->lg_ms[0] = group_ms;
    if (K) ctx->dc_ms[0] = group_ms;
    if (CS) ctx->cost_ms[0] = cost_ms;
    if (stats) {
        acc.schedule = ctx->sched;
        acc.samples = counted * p->spp;
        if (ctx->counters) {
            unsigned long long c[8];
            HIPCHK(hipMemcpy(c, d_counters, sizeof(c), hipMemcpyDeviceToHost));
            acc.rays_extend = c[0];
            acc.rays_shadow = c[1];
            acc.node_visits = c[2];
            acc.tri_tests = c[3];
            acc.bounces = c[4];
            acc.octree_checks = c[5];
            acc.octree_replays = c[6];
        }
        add_stats(*stats, acc, Times::Sum);
    }
    return NART_OK;
}

// ---------------------------------------------------------------- device-side BVH build
struct LbvhResult {
    uint32_t max_stack = 1, num_nodes = 0, num_leaf_tris = 0;
    int32_t root_code = -1;
};

// Linear BVH on the device (device/lbvh.h) over the triangles the reference octree can return
// (mask), into ctx->d_nodes / d_tri_isect / d_tri_perm.  ctx->d_tris must be resident.
int build_bvh_device(nart_ctx* ctx, const nart_scene_blob& blob, const std::vector<uint8_t>& mask,
                     const nart::RefOctree& oct, float pad, float margin, LbvhResult& out) {
    std::vector<uint32_t> vis, info;
    for (uint32_t g = 0; g < blob.num_triangles; ++g)
        if (mask[g]) vis.push_back(g);
    nart::octree_leaf_info(blob, oct, margin, info);
    const uint32_t m = (uint32_t)vis.size();
    out.num_leaf_tris = m;
    if (m == 0) {  // nothing the octree can return: never traversed (geometry_visible = 0)
        BVHNode dummy{};
        int rc = upload(ctx, ctx->d_nodes, &dummy, 0, "BVH nodes");
        if (!rc) rc = upload(ctx, ctx->d_tri_isect, (const float*)nullptr, 0, "triangle records");
        if (!rc) rc = upload(ctx, ctx->d_tri_perm, (const float*)nullptr, 0, "permuted triangle records");
        return rc;
    }
    const int n = (int)((m + LBVH_LEAF - 1) / LBVH_LEAF);  // leaves
    const int ninner = n - 1;
    std::vector<Buf> tmp;  // the build's scratch, freed on every return path
    auto alloc = [&](auto*& p, size_t bytes) {
        tmp.emplace_back();
        const int rc = reserve(ctx, tmp.back(), ctx->device, bytes ? bytes : 4, "BVH build scratch");
        p = tmp.back().as<std::remove_reference_t<decltype(*p)>>();
        return rc;
    };
    uint32_t *d_vis, *d_info, *d_keys[2], *d_vals[2], *d_lkey, *d_flag, *d_maxd, *d_ord[2];
    LbvhPrim *d_prims, *d_sorted;
    float* d_part;
    int2* d_child;
    int *d_pin, *d_pleaf, *d_remap;
    LbvhBox* d_box;
    const uint32_t nb = std::min<uint32_t>(1024, (m + 255) / 256);
    const size_t ni = (size_t)std::max(ninner, 1);
    int rc = NART_OK;
    if ((rc = alloc(d_vis, m * 4)) || (rc = alloc(d_info, blob.num_triangles * 4)) ||
        (rc = alloc(d_prims, m * sizeof(LbvhPrim))) || (rc = alloc(d_sorted, m * sizeof(LbvhPrim))) ||
        (rc = alloc(d_part, nb * 6 * 4)) || (rc = alloc(d_keys[0], m * 4)) ||
        (rc = alloc(d_keys[1], m * 4)) || (rc = alloc(d_vals[0], m * 4)) ||
        (rc = alloc(d_vals[1], m * 4)) || (rc = alloc(d_lkey, n * 4)) ||
        (rc = alloc(d_child, ni * sizeof(int2))) || (rc = alloc(d_pin, ni * 4)) ||
        (rc = alloc(d_pleaf, (size_t)n * 4)) || (rc = alloc(d_box, ni * sizeof(LbvhBox))) ||
        (rc = alloc(d_flag, ni * 4)) || (rc = alloc(d_maxd, 4)) ||
        (rc = alloc(d_ord[0], ni * 4)) || (rc = alloc(d_ord[1], ni * 4)) ||
        (rc = alloc(d_remap, ni * 4)))
        return rc;
    if (hipMemcpy(d_vis, vis.data(), m * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_info, info.data(), blob.num_triangles * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_pin, 0xFF, ni * 4) != hipSuccess || hipMemset(d_pleaf, 0xFF, (size_t)n * 4) != hipSuccess ||
        hipMemset(d_flag, 0, ni * 4) != hipSuccess || hipMemset(d_maxd, 0, 4) != hipSuccess)
        return fail(ctx, NART_E_HIP, "BVH build: upload");
    const dim3 blk(256);
    const uint32_t gm = (m + 255) / 256, gn = ((uint32_t)n + 255) / 256, gi = ((uint32_t)ni + 255) / 256;
    hipLaunchKernelGGL(k_lbvh_prims, dim3(gm), blk, 0, 0, ctx->d_tris.as<const nart_triangle>(), d_vis, m, d_prims);
    hipLaunchKernelGGL(k_lbvh_bounds, dim3(nb), blk, 0, 0, d_prims, m, d_part);
    hipLaunchKernelGGL(k_lbvh_bounds_final, dim3(1), dim3(64), 0, 0, d_part, nb);
    hipLaunchKernelGGL(k_lbvh_morton, dim3(gm), blk, 0, 0, d_prims, m, d_part, d_keys[0], d_vals[0]);
    size_t ts = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, ts, d_keys[0], d_keys[1], d_vals[0], d_vals[1], (int)m, 0, 30) !=
        hipSuccess)
        return fail(ctx, NART_E_HIP, "BVH build: sort size");
    char* d_ts = nullptr;
    if ((rc = alloc(d_ts, ts))) return rc;
    if (hipcub::DeviceRadixSort::SortPairs(d_ts, ts, d_keys[0], d_keys[1], d_vals[0], d_vals[1], (int)m, 0, 30) !=
        hipSuccess)
        return fail(ctx, NART_E_HIP, "BVH build: sort");
    hipLaunchKernelGGL(k_lbvh_gather, dim3(gm), blk, 0, 0, d_prims, d_vals[1], m, d_sorted);
    hipLaunchKernelGGL(k_lbvh_leaf_keys, dim3(gn), blk, 0, 0, d_keys[1], m, n, d_lkey);
    if (ninner > 0) {
        hipLaunchKernelGGL(k_lbvh_karras, dim3(gi), blk, 0, 0, d_lkey, n, d_child, d_pin, d_pleaf);
        hipLaunchKernelGGL(k_lbvh_refit, dim3(gn), blk, 0, 0, d_sorted, m, n, d_child, d_pin, d_pleaf, d_box, d_flag);
        hipLaunchKernelGGL(k_lbvh_depth, dim3(gi), blk, 0, 0, d_pin, ninner, d_keys[0], d_vals[0], d_maxd);
        size_t ts2 = 0;
        if (hipcub::DeviceRadixSort::SortPairs(nullptr, ts2, d_keys[0], d_keys[1], d_vals[0], d_ord[0], ninner, 0, 8) !=
            hipSuccess)
            return fail(ctx, NART_E_HIP, "BVH build: sort size");
        char* d_ts2 = nullptr;
        if ((rc = alloc(d_ts2, ts2))) return rc;
        if (hipcub::DeviceRadixSort::SortPairs(d_ts2, ts2, d_keys[0], d_keys[1], d_vals[0], d_ord[0], ninner, 0, 8) !=
            hipSuccess)
            return fail(ctx, NART_E_HIP, "BVH build: sort");
        hipLaunchKernelGGL(k_lbvh_remap, dim3(gi), blk, 0, 0, d_ord[0], ninner, d_remap);
    }
    if ((rc = reserve(ctx, ctx->d_nodes, ctx->device, ni * sizeof(BVHNode), "BVH nodes")) ||
        (rc = reserve(ctx, ctx->d_tri_isect, ctx->device, (size_t)m * 64, "triangle records")) ||
        (rc = reserve(ctx, ctx->d_tri_perm, ctx->device, ((size_t)m * 3 + NART_TRI_PAD) * 64, "permuted triangle records")))
        return rc;
    if (ninner > 0)
        hipLaunchKernelGGL(k_lbvh_emit, dim3(gi), blk, 0, 0, d_ord[0], ninner, d_child, d_remap, d_box, d_sorted, m, pad,
                           ctx->d_nodes.as<BVHNode>());
    hipLaunchKernelGGL(k_lbvh_tris, dim3(gm), blk, 0, 0, ctx->d_tris.as<const nart_triangle>(), d_sorted, m, d_info,
                       ctx->d_tri_isect.as<float>());
    hipLaunchKernelGGL(k_lbvh_perm, dim3(gm), blk, 0, 0, ctx->d_tri_isect.as<const float>(), m, ctx->d_tri_perm.as<float>());
    uint32_t maxd = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpy(&maxd, d_maxd, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ctx, NART_E_HIP, "BVH build: kernels");
    out.num_nodes = (uint32_t)std::max(ninner, 0);
    out.max_stack = ninner > 0 ? maxd + 1 : 1;
    out.root_code = ninner > 0 ? 0 : ~(int32_t)(m - 1);  // one leaf of m <= LBVH_LEAF triangles
    return NART_OK;
}

// ---------------------------------------------------------------- whole frames
// One adaptive render (include/nart_hip.h, "Adaptive sampling"): the validated parameters and the
// level list going in; coming out, per bucket (in the order of the list rendered: bucket-id order for
// a whole frame) the sample count it ended on and the error of that level, the buckets rendered per
// level, and the device times of the error and scatter kernels and of the levels' passes.
struct AdaptiveRun {
    nart_adaptive_params ap;
    std::vector<uint32_t> levels;
    std::vector<uint32_t> spp;
    std::vector<float> err;
    std::vector<uint32_t> rendered;
    double ms = 0.0;
    PassTimes passes;
};

// Where the images of a whole frame go and whose buffers it uses (render_frame); what the frame
// produces is its FramePlan, and everything here that counts outputs follows the plan's list.
struct FrameRequest {
    // Delivery: the image of output i to the host at dst[i] (null: rendered, not delivered); or
    // on_device, the images of the plan's outputs back to back, in list order, from the start of
    // *image on device 0 (ordered on its null stream: single-device frames do not wait for them).
    nart_pixel* dst[FRAME_MAX_OUTPUTS] = {};
    bool on_device = false;
    // The call's tile and image buffers.  image null: temporaries, allocated by the call and freed on
    // every return path.  Else borrowed from a context, which keeps them for its next call (the
    // memory a context holds between calls sets batch_slot_limit): the image buffer *image on
    // device 0, grown to max(images, outputs) images; tiles in d_gather.  A
    // multi-device context always gathers and combines in its own cached buffers.
    Buf* image = nullptr;
    uint32_t images = 0;
    // With plan.ask.adaptive (every device refines its own buckets): the run's parameters and results.
    AdaptiveRun* adaptive = nullptr;

    FrameRequest() = default;
    FrameRequest(Buf* image_, uint32_t n) : on_device(true), image(image_), images(n) {}
    // `img` is where the plan's output of `kind` goes on the host (a failed plan has no outputs).
    void to_host(const FramePlan& plan, OutputKind kind, nart_pixel* img) {
        const int i = plan.find(kind);
        if (i >= 0) dst[i] = img;
    }
};

// ---------------------------------------------------------------- adaptive sampling (device/adaptive.h)
// The adaptive counterpart of render_buckets: the listed buckets, refined level by level, into the
// frame's tile buffers (list order: slot i is ids[i]).  Every level renders its list at that level's
// sample count into list-ordered scratch tiles -- the outputs of adaptive_level_ask: what the frame
// asks for and, wanted or not, the second-moment tiles -- k_bucket_error reduces each bucket's beauty
// and moment tiles to its error, k_scatter_tiles moves the frame's outputs' tiles to their slots
// (replacing the earlier level's: a pixel's RNG stream is seeded by its coordinates, so a second pass
// would replay the first one's numbers and must not be accumulated), and the buckets whose error is
// not <= threshold form the next list.  A bucket's tiles are therefore those of a uniform render at
// the sample count it ended on.  The scratch is a temporary of the call.  p and run.ap are validated
// by the caller; run.levels is set.
int render_buckets_adaptive(nart_ctx* ctx, const nart_render_params* p, const uint32_t* ids, uint32_t n,
                            const FrameTiles& frame, hipStream_t st, nart_render_stats* stats, AdaptiveRun& run) {
    HIPCHK(hipSetDevice(ctx->device));
    const FramePlan level = plan_frame(adaptive_level_ask(frame.plan.ask), PlanRules::Buckets);
    if (level.code) return fail(ctx, level.code, level.message);
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    const size_t tile_floats = (size_t)g.tile_size * g.tile_size * 5;
    run.spp.assign(n, 0);
    run.err.assign(n, 0.f);
    run.rendered.assign(run.levels.size(), 0);
    if (!n) return NART_OK;
    Buf own_tiles, own_lists;  // freed on return
    const size_t slab = (size_t)n * tile_floats;
    int rc = reserve(ctx, own_tiles, ctx->device, level.n_outputs * slab * sizeof(float), "adaptive scratch tiles");
    if (!rc) rc = reserve(ctx, own_lists, ctx->device, (size_t)n * 12, "adaptive bucket lists");
    if (rc) return rc;
    const FrameTiles scratch(level, own_tiles.as<float>(), slab);
    uint32_t* d_ids = own_lists.as<uint32_t>();
    uint32_t* d_slot = d_ids + n;
    float* d_err = reinterpret_cast<float*>(d_slot + n);

    std::vector<uint32_t> cur(n), cur_ids, next;  // slots of the current list, ascending
    for (uint32_t i = 0; i < n; ++i) cur[i] = i;
    std::vector<float> E;
    const size_t stage_lds = (2 * (size_t)p->bucket_size * (p->bucket_size + 1) + 2 * (size_t)p->bucket_size) * sizeof(float);
    const bool stage = stage_lds <= 64 * 1024;
    if ((size_t)p->bucket_size * 2 * sizeof(float) > 64 * 1024)
        return fail(ctx, NART_E_UNSUPPORTED, "adaptive sampling: bucket rows do not fit the LDS");
    for (size_t li = 0; li < run.levels.size() && !cur.empty(); ++li) {
        const uint32_t m = (uint32_t)cur.size();
        const bool last = li + 1 == run.levels.size();
        nart_render_params pl = *p;
        pl.spp = run.levels[li];
        cur_ids.resize(m);
        for (uint32_t i = 0; i < m; ++i) cur_ids[i] = ids[cur[i]];
        rc = render_buckets(ctx, &pl, cur_ids.data(), m, scratch, st, stats, &run.passes);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(d_ids, cur_ids.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_slot, cur.data(), (size_t)m * 4, hipMemcpyHostToDevice, st));
        BucketErrorArgs ea;
        ea.beauty = scratch.of(OutputKind::Beauty);
        ea.moment = scratch.of(OutputKind::Moment);
        ea.ids = d_ids;
        ea.err = d_err;
        ea.n = m;
        ea.B = p->bucket_size;
        ea.fb = g.filter_bounds;
        ea.tile = g.tile_size;
        ea.nbx = g.n_buckets_x;
        ea.totalW = g.total_width;
        ea.totalH = g.total_height;
        ea.floor = run.ap.floor;
        ScatterArgs sc = {};  // (unused buffers null)
        uint32_t nsc = 0;
        for (uint32_t o = 0; o < frame.plan.n_outputs && nsc < (uint32_t)SCATTER_BUFS; ++o) {
            sc.src[nsc] = scratch.of(frame.plan.outputs[o].kind);
            sc.dst[nsc++] = frame.tiles[o];
        }
        sc.slot = d_slot;
        sc.n = m;
        sc.tile_floats = (uint32_t)tile_floats;
        double ms = 0.0;
        rc = timed(ctx, ctx->ev_ad, st, &ms, [&]() -> int {
            if (stage) hipLaunchKernelGGL((k_bucket_error<true>), dim3(m), dim3(64), stage_lds, st, ea);
            else hipLaunchKernelGGL((k_bucket_error<false>), dim3(m), dim3(64), 2 * (size_t)p->bucket_size * sizeof(float), st, ea);
            HIPCHK(hipGetLastError());
            if (nsc) {
                hipLaunchKernelGGL(k_scatter_tiles, dim3(m, nsc), dim3(256), 0, st, sc);
                HIPCHK(hipGetLastError());
            }
            return NART_OK;
        });
        if (rc) return rc;
        run.ms += ms;
        E.resize(m);
        HIPCHK(hipMemcpyAsync(E.data(), d_err, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        run.rendered[li] = m;
        next.clear();
        for (uint32_t i = 0; i < m; ++i) {
            run.spp[cur[i]] = run.levels[li];
            run.err[cur[i]] = E[i];
            if (!last && !(E[i] <= run.ap.threshold)) next.push_back(cur[i]);  // a NaN error refines
        }
        cur.swap(next);
    }
    return NART_OK;
}

}  // namespace

#include "host/multi_gpu.h"

namespace {

// Render(): every bucket of the session, combined in bucket raster order, delivered as the request
// says.  The one whole-frame path behind nart_hip_render, _render_aovs, _render_moment,
// _render_adaptive, _render_device, _render_denoised, _render_cascade and _render_mattes: `plan` is
// plan_frame(ask, PlanRules::Frame) of the entry point's ask, its error raised here.  times: the passes'
// device times.  Errors of a multi-device context's sub-contexts are re-raised on ctx.
int render_frame(nart_ctx* ctx, const nart_render_params* p, const FramePlan& plan, const FrameRequest& rq,
                 nart_render_stats* stats, PassTimes* times = nullptr) {
    RenderTimer timer(stats);
    PassTimes unused;
    if (!times) times = &unused;
    *times = PassTimes();
    if (plan.code) return fail(ctx, plan.code, plan.message);
    nart_ctx* c0 = first_device(ctx);  // device 0: combines, holds the images
    int rc = NART_OK;
    if (ctx->rccl_broken)
        return fail(ctx, NART_E_RCCL, "an earlier RCCL gather of this context failed; destroy it and create a new one");
    if ((rc = forwarded(ctx, check_params(c0, p)))) return rc;
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    const uint32_t nb = g.n_buckets_x * g.n_buckets_y;
    const size_t tile_floats = (size_t)nb * g.tile_size * g.tile_size * 5;
    const size_t img_floats = (size_t)g.total_width * g.total_height * 5;
    const size_t K = plan.n_outputs;
    if (rq.image &&
        (rc = reserve(ctx, *rq.image, c0->device, std::max<size_t>(K, rq.images) * img_floats * sizeof(float), "image")))
        return rc;
    if (c0 != ctx) return render_multi(ctx, p, plan, rq, stats, *times);

    HIPCHK(hipSetDevice(ctx->device));
    // the outputs' tile buffers back to back; one image to combine into on the way to the host, or
    // the borrowed images
    Buf own_tiles, own_img;  // freed on return
    Buf& tiles = rq.image ? ctx->d_gather : own_tiles;
    Buf& image = rq.image ? *rq.image : own_img;
    rc = reserve(ctx, tiles, ctx->device, K * tile_floats * sizeof(float), "tiles");
    if (!rc && !rq.image) rc = reserve(ctx, image, ctx->device, img_floats * sizeof(float), "image");
    if (rc) return rc;
    const FrameTiles out(plan, tiles.as<float>(), tile_floats);
    std::vector<uint32_t> ids(nb);
    for (uint32_t i = 0; i < nb; ++i) ids[i] = i;
    if (rq.adaptive) {
        rc = render_buckets_adaptive(ctx, p, ids.data(), nb, out, 0, stats, *rq.adaptive);
        *times = rq.adaptive->passes;
    } else {
        rc = render_buckets(ctx, p, ids.data(), nb, out, 0, stats, times);
    }
    for (size_t i = 0; i < K && !rc; ++i) {
        if (!rq.on_device && !rq.dst[i]) continue;
        float* img = image.as<float>() + (rq.on_device ? i * img_floats : 0);
        rc = nart_hip_combine_async(ctx, p, reinterpret_cast<const nart_pixel*>(out.tiles[i]),
                                    reinterpret_cast<nart_pixel*>(img), 0);
        if (rc || rq.on_device) continue;
        if (hipMemcpy(rq.dst[i], img, img_floats * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, NART_E_HIP, "copy image");
    }
    return rc;
}

// Slots of the per-sample entry points: one per pixel of a rect in total-image coordinates, row by
// row, each pixel's samples a row of their own (k_slot_rows), on the null stream.  p is validated
// by the caller.  An empty rect gives no slots: what then is the caller's to say.
int rect_slots(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
               unsigned long long* counters, RenderArgs& ra) {
    HIPCHK(hipSetDevice(ctx->device));
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    // in 64 bits: x0 + w may wrap in 32
    if ((uint64_t)x0 + w > g.total_width || (uint64_t)y0 + h > g.total_height)
        return fail(ctx, NART_E_INVALID, "rect out of range");
    std::vector<uint32_t> xy;
    append_rect(xy, x0, y0, w, h);
    const uint32_t n = (uint32_t)xy.size();
    if (int rc = ensure(ctx, n, p->spp, 1)) return rc;
    HIPCHK(hipMemcpy(ctx->d_slot_xy.as<uint32_t>(), xy.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_slot_rows, dim3((n + 255) / 256), dim3(256), 0, 0, n, p->spp, ctx->d_slot_so.as<SlotSO>());
    ctx->rows_pixel_major = true;
    ra = make_render_args(ctx, p, g, n, counters);
    return NART_OK;
}

// The group of every light (validated by the caller: light_groups_error) onto every device of ctx,
// for the light-group renders that follow (render_buckets reads it where the plan has groups).
int set_light_groups(nart_ctx* ctx, const uint32_t* group_of_light) {
    for (nart_ctx* c : ctx->subs)
        if (int rc = set_light_groups(c, group_of_light)) return fail(ctx, rc, c->err);
    if (!ctx->subs.empty()) return NART_OK;
    HIPCHK(hipSetDevice(ctx->device));
    return upload(ctx, ctx->d_light_group, group_of_light, ctx->scene.num_lights, "light groups");
}

// The cuts (validated by the caller: depth_cuts_error) onto every device's context of ctx, for the
// depth-cut renders that follow (render_buckets hands them to the path kernel in its arguments).
void set_depth_cuts(nart_ctx* ctx, const uint32_t* cuts, uint32_t K) {
    for (nart_ctx* c : ctx->subs) set_depth_cuts(c, cuts, K);
    for (uint32_t j = 0; j < DEPTH_CUTS_MAX; ++j) ctx->depth_cuts[j] = j < K ? cuts[j] : 0u;
    ctx->n_depth_cuts = K;
}

}  // namespace

#include "host/image_stages.h"

namespace {

// Largest coordinate magnitude of the scene (triangles and camera position; at least 1): the scale
// of the BVH box padding and of the octree margins (nart_hip_create, nart_hip_bvh_dump).
float scene_maxabs(const nart_scene_blob& blob) {
    float maxabs = 1.f;
    for (uint32_t g = 0; g < blob.num_triangles; ++g) {
        const nart_triangle& T = blob.triangles[g];
        for (int k = 0; k < 3; ++k)
            maxabs = std::max(maxabs, std::max(std::fabs(T.v0[k]), std::max(std::fabs(T.v1[k]), std::fabs(T.v2[k]))));
    }
    for (int k = 12; k < 15; ++k) maxabs = std::max(maxabs, std::fabs(blob.camera.m[k]));
    for (int k = 3; k < 16; k += 4) maxabs = std::max(maxabs, std::fabs(blob.camera.m[k]));
    return maxabs;
}

// vertex block of every triangle test record, permuted for each ray major axis, followed
// by the plane {n, dot(v0, n)}: one 64-B record, so a test issues its four loads at once
void permute_tri_records(const std::vector<float>& tri_isect, std::vector<float>& perm) {
    const size_t nt = tri_isect.size() / 16;
    perm.assign((3 * nt + NART_TRI_PAD) * 16, 0.f);  // + padding records (trav_step's record groups)
    for (int m = 0; m < 3; ++m) {
        const int kx = (m + 1) % 3, ky = (m + 2) % 3, kz = m;
        for (size_t i = 0; i < nt; ++i) {
            const float* r = &tri_isect[i * 16];
            const float* v[3] = {r + 4, r + 7, r + 10};  // v0, v1, v2 (words 4-12)
            float* o = &perm[((size_t)m * nt + i) * 16];
            for (int k = 0; k < 3; ++k) {
                o[3 * k + 0] = v[k][kx];
                o[3 * k + 1] = v[k][ky];
                o[3 * k + 2] = v[k][kz];
            }
            o[9] = r[13];   // global index
            o[10] = r[14];  // octree leaf | inside bit
            o[11] = r[15];  // grazing threshold
            for (int k = 0; k < 4; ++k) o[12 + k] = r[k];  // plane (words 0-3)
        }
    }
}

// nart_hip_bvh_dump / nart_hip_context_bvh_dump: the sizes, and whether the caller's buffers hold them
// (all three null: a size query)
int bvh_dump_check(const nart_bvh_dump_info& info, const void* nodes, size_t nodes_cap, const float* tri_isect,
                   size_t isect_cap, const float* tri_perm, size_t perm_cap) {
    if (!nodes && !tri_isect && !tri_perm) return 1;
    if (!nodes || !tri_isect || !tri_perm) return NART_E_INVALID;
    if (nodes_cap < info.num_nodes || isect_cap < (size_t)info.num_leaf_tris * 16 ||
        perm_cap < (size_t)info.num_leaf_tris * 48)
        return NART_E_INVALID;
    return NART_OK;
}

}  // namespace

extern "C" {

int nart_hip_create(const nart_scene_blob* blob, int device_id, nart_ctx** out) {
    if (!blob || !out) return NART_E_INVALID;
    nart_ctx* ctx = new (std::nothrow) nart_ctx();
    if (!ctx) return NART_E_OOM;
    *out = nullptr;
    ctx->device = device_id;
    if (const char* v = env_opt("NART_VARIANT")) {
        const int var = std::atoi(v);
        if (var == 0 || var == 3) ctx->variant = var;
    }
    if (const char* v = env_opt("NART_SPLAT_MODE")) ctx->splat_mode = std::max(-1, std::min(5, std::atoi(v)));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id || device_id < 0) {
        delete ctx;
        return NART_E_HIP;
    }
    int rc = NART_OK;
    auto bail = [&](int code) {
        delete ctx;
        return code;
    };
    if (hipSetDevice(device_id) != hipSuccess) return bail(NART_E_HIP);
    // dynamic LDS above the 64 KiB default: LatinSquare arrays (128 KiB at 256 spp)
    if (hipFuncSetAttribute((const void*)k_latin_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return bail(NART_E_HIP);
    if (hipFuncSetAttribute((const void*)k_latin_idx, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
        return bail(NART_E_HIP);
    if (hipFuncSetAttribute((const void*)k_latin_perm<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess ||
        hipFuncSetAttribute((const void*)k_latin_perm<80>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess ||
        hipFuncSetAttribute((const void*)k_latin_emit, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
        return bail(NART_E_HIP);
    // reference octree visibility (Q14) + device BVH
    std::vector<uint8_t> mask;
    bool root_leaf = false;
    uint32_t n_chunks = 0;
    nart::RefOctree oct;
    nart::reference_visibility(*blob, mask, root_leaf, n_chunks, &oct);
    const float maxabs = scene_maxabs(*blob);
    // hit points deviate from the reference's slab arithmetic by far less than 2^-14 * scene
    // scale (|o| + |t d| <= 3 * maxabs, errors of a few ulps): octree.h oc_clear
    const float pad = maxabs * 6.103515625e-05f + 1e-6f, margin = maxabs * 6.103515625e-05f;
    if ((rc = upload(ctx, ctx->d_tris, blob->triangles, blob->num_triangles, "triangles"))) return bail(rc);
    // NART_BVH_BUILD=device: linear BVH built on the GPU (device/lbvh.h); default: binned SAH on
    // the host (host/bvh_build.cpp) -- same node / record format, same images
    const char* bb = env_opt("NART_BVH_BUILD");
    ctx->bvh_on_device = bb && std::string(bb) == "device";
    const auto tb0 = std::chrono::steady_clock::now();
    LbvhResult lb;
    if (ctx->bvh_on_device) {
        if ((rc = build_bvh_device(ctx, *blob, mask, oct, pad, margin, lb))) return bail(rc);
    } else {
        nart::BuiltBVH bvh;
        nart::build_bvh(*blob, mask, pad, bvh);
        nart::annotate_octree_leaves(*blob, oct, margin, bvh);
        lb.max_stack = bvh.max_stack;
        lb.num_nodes = (uint32_t)bvh.nodes.size();
        lb.root_code = bvh.root_code;
        lb.num_leaf_tris = (uint32_t)(bvh.tri_isect.size() / 16);
        if ((rc = upload(ctx, ctx->d_nodes, bvh.nodes.data(), bvh.nodes.size(), "BVH nodes"))) return bail(rc);
        if ((rc = upload(ctx, ctx->d_tri_isect, bvh.tri_isect.data(), bvh.tri_isect.size(), "triangle records")))
            return bail(rc);
        std::vector<float> perm;
        permute_tri_records(bvh.tri_isect, perm);
        if ((rc = upload(ctx, ctx->d_tri_perm, perm.data(), perm.size(), "permuted triangle records"))) return bail(rc);
    }
    ctx->bvh_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count();
    ctx->stack_depth = std::max<uint32_t>(lb.max_stack + 1, 2);
    if ((size_t)ctx->stack_depth * 256 * 8 > (size_t)160 * 1024) return bail(NART_E_UNSUPPORTED);  // LDS stack
    ctx->num_nodes = lb.num_nodes;
    ctx->num_leaf_tris = lb.num_leaf_tris;
    ctx->root_code = lb.root_code;
    ctx->bvh_pad = pad;
    std::vector<uint32_t> tri_mesh(blob->num_triangles);
    std::vector<DMesh> meshes(blob->num_meshes);
    for (uint32_t m = 0; m < blob->num_meshes; ++m) {
        meshes[m].material = blob->meshes[m].material;
        meshes[m].priority = blob->meshes[m].priority & 0xFFu;
        for (uint32_t i = 0; i < blob->meshes[m].num_tris; ++i) tri_mesh[blob->meshes[m].first_tri + i] = m;
    }
    if (blob->num_meshes >= (1u << 24)) return bail(NART_E_UNSUPPORTED);
    if ((rc = upload(ctx, ctx->d_tri_mesh, tri_mesh.data(), tri_mesh.size(), "triangle meshes"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_meshes, meshes.data(), meshes.size(), "meshes"))) return bail(rc);
    ctx->num_meshes = blob->num_meshes;
    ctx->num_materials = blob->num_materials;
    std::vector<DMaterial> mats(blob->num_materials);
    for (uint32_t i = 0; i < blob->num_materials; ++i) {
        const nart_material& m = blob->materials[i];
        DMaterial& d = mats[i];
        d.type = m.type;
        d.has_normal = (m.type == NART_MAT_GLASS) ? 0 : m.has_normal;  // glassmaterial.cpp:3-9
        d.rho_d = dpat(m.rho_d);
        d.rho_s = dpat(m.rho_s);
        d.tau = dpat(m.tau);
        d.eta = dpat(m.eta);
        d.alpha = dpat(m.alpha);
        d.normal = dpat(m.normal);
    }
    if ((rc = upload(ctx, ctx->d_mats, mats.data(), mats.size(), "materials"))) return bail(rc);
    // per mesh: bxdf_eta of its one-lobe constant-pattern BSDF (the compact dielectric list,
    // kernels.h IList): B_LAMBERT -> 0, every other one-lobe kind -> the material's eta value
    std::vector<float> mesh_eta(blob->num_meshes);
    for (uint32_t m = 0; m < blob->num_meshes; ++m) {
        const uint32_t mi = blob->meshes[m].material;
        mesh_eta[m] = (mi >= mats.size() || mats[mi].type == NART_MAT_LAMBERT) ? 0.f : mats[mi].eta.v[0];
    }
    if ((rc = upload(ctx, ctx->d_mesh_eta, mesh_eta.data(), mesh_eta.size(), "mesh etas"))) return bail(rc);
    std::vector<DLight> lights;
    std::vector<DEnvDist> envs;
    for (uint32_t l = 0; l < blob->num_lights; ++l) {
        lights.push_back(dlight(blob->lights[l]));
        const nart_light& L = blob->lights[l];
        if (L.type == NART_LIGHT_ENVIRONMENT) ctx->has_env = true;
        if (L.type == NART_LIGHT_ENVIRONMENT && L.Le.type == NART_PTN_TEXTURE) {
            DEnvDist d;
            if ((rc = build_env(ctx, blob->textures[L.Le.texture], d))) return bail(rc);
            lights.back().env = (int32_t)envs.size();
            envs.push_back(d);
            ctx->env_dims.push_back(d.w);
            ctx->env_dims.push_back(d.h);
        }
    }
    if ((rc = upload(ctx, ctx->d_envs, envs.data(), envs.size(), "environment distributions"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_lights, lights.data(), lights.size(), "lights"))) return bail(rc);
    ctx->lights = lights;
    ctx->features = scene_features(blob);
    std::vector<DTexture> texs(blob->num_textures);
    ctx->num_textures = blob->num_textures;
    size_t pool = 0;
    for (uint32_t t = 0; t < blob->num_textures; ++t) {
        texs[t].w = blob->textures[t].width;
        texs[t].h = blob->textures[t].height;
        texs[t].offset = pool;
        pool += (size_t)texs[t].w * texs[t].h * 4;
    }
    std::vector<uint16_t> tex_pool(pool ? pool : 1);
    for (uint32_t t = 0; t < blob->num_textures; ++t)
        std::memcpy(&tex_pool[texs[t].offset], blob->textures[t].rgba, (size_t)texs[t].w * texs[t].h * 8);
    if ((rc = upload(ctx, ctx->d_texs, texs.data(), texs.size(), "textures"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_tex_pool, tex_pool.data(), tex_pool.size(), "texels"))) return bail(rc);

    DScene& S = ctx->scene;
    std::memset(&S, 0, sizeof(S));
    S.nodes = ctx->d_nodes.as<const BVHNode>();
    S.tri_isect = ctx->d_tri_isect.as<const float4>();
    S.tri_perm = ctx->d_tri_perm.as<const float4>();
    S.tris = ctx->d_tris.as<const nart_triangle>();
    S.tri_mesh = ctx->d_tri_mesh.as<const uint32_t>();
    S.meshes = ctx->d_meshes.as<const DMesh>();
    S.mats = ctx->d_mats.as<const DMaterial>();
    S.mesh_eta = ctx->d_mesh_eta.as<const float>();
    S.lights = ctx->d_lights.as<const DLight>();
    S.texs = ctx->d_texs.as<const DTexture>();
    S.tex_pool = ctx->d_tex_pool.as<const uint16_t>();
    S.envs = ctx->d_envs.as<const DEnvDist>();
    if ((rc = build_medium(ctx, blob->medium, S.medium))) return bail(rc);
    S.num_lights = blob->num_lights;
    S.num_tris = blob->num_triangles;
    S.num_leaf_tris = lb.num_leaf_tris;
    S.root = lb.root_code;
    S.geometry_visible = (!root_leaf && lb.num_leaf_tris > 0) ? 1 : 0;
    std::memcpy(S.cam_m, blob->camera.m, sizeof(S.cam_m));
    // glm::tan(glm::radians(fov)) with the host libm, as the reference (pinholecamera.cpp:20)
    S.cam_tan = std::tan(blob->camera.fov * (float)0.01745329251994329576923690768489);
    // reference octree + replay heap pool: entries of 64 heaps (one per lane of a replaying
    // wave, octree.h oc_replay), held only while a wave replays; up to 512 entries within 256 MiB
    // (NART_OC_POOL overrides the count: tests force a single entry)
    if ((rc = upload(ctx, ctx->d_oc_nodes, oct.nodes.data(), oct.nodes.size(), "octree nodes"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_oc_chunks, oct.chunks.data(), oct.chunks.size(), "octree chunks"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_oc_tris, oct.tris.data(), oct.tris.size(), "octree triangles"))) return bail(rc);
    if ((rc = upload(ctx, ctx->d_tri_leaf, oct.tri_leaf.data(), oct.tri_leaf.size(), "triangle leaves"))) return bail(rc);
    S.oc_nodes = ctx->d_oc_nodes.as<const OcNode>();
    S.oc_chunks = ctx->d_oc_chunks.as<const uint32_t>();
    S.oc_tris = ctx->d_oc_tris.as<const uint32_t>();
    S.tri_leaf = ctx->d_tri_leaf.as<const int32_t>();
    S.oc_root = oct.root;
    S.oc_cap = (uint32_t)std::max<size_t>(oct.nodes.size(), 1);
    S.oc_pool = (uint32_t)std::max<size_t>(1, std::min<size_t>(512, (256ull << 20) / (64ull * 8ull * S.oc_cap)));
    if (const char* v = env_opt("NART_OC_POOL")) S.oc_pool = (uint32_t)std::max(1, std::atoi(v));
    S.oc_scale = maxabs;
    S.oc_exact = 1;
    // NART_OCTREE_EXACT: 0 off (A/B timing only), 2 every query replays the octree search (tests)
    if (const char* v = env_opt("NART_OCTREE_EXACT")) S.oc_exact = std::max(0, std::min(2, std::atoi(v)));
    if (reserve(ctx, ctx->d_oc_lock, ctx->device, sizeof(uint32_t) * S.oc_pool, "octree replay locks") ||
        hipMemset(ctx->d_oc_lock.as<void>(), 0, sizeof(uint32_t) * S.oc_pool) != hipSuccess ||
        reserve(ctx, ctx->d_oc_heap, ctx->device, sizeof(unsigned long long) * 64 * S.oc_pool * S.oc_cap,
                "octree replay heaps"))
        return bail(NART_E_OOM);
    S.oc_lock = ctx->d_oc_lock.as<uint32_t>();
    S.oc_heap = ctx->d_oc_heap.as<unsigned long long>();
    *out = ctx;
    return NART_OK;
}

// The context's buffers, events and streams free themselves (host/device_buf.h).
void nart_hip_destroy(nart_ctx* ctx) {
    if (!ctx) return;
    for (ncclComm_t c : ctx->comms)
        if (c && rccl_api().ok) rccl_api().CommDestroy(c);
    for (nart_ctx* c : ctx->subs) nart_hip_destroy(c);
    delete ctx;
}

const char* nart_hip_last_error(const nart_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int nart_hip_set_counters(nart_ctx* ctx, int enable) {
    if (!ctx) return NART_E_INVALID;
    ctx->counters = enable != 0;
    for (nart_ctx* c : ctx->subs) c->counters = ctx->counters;
    return NART_OK;
}

int nart_hip_set_splat_mode(nart_ctx* ctx, int mode) {
    if (!ctx) return NART_E_INVALID;
    for (nart_ctx* c : ctx->subs)
        if (int rc = nart_hip_set_splat_mode(c, mode)) return fail(ctx, rc, c->err);
    if (mode < -1 || mode > 5)
        return fail(ctx, NART_E_UNSUPPORTED, "splat mode must be -1 (automatic) or 0-5 (5 skewed-time tile rows, 4 skewed-time "
                                             "tile columns, 3 four pixels per lane, 1-0 one pixel per lane; the "
                                             "LDS-staged and tile-column-sweep modes were retired, DESIGN.md)");
    ctx->splat_mode = mode;
    return NART_OK;
}

int nart_hip_set_specialize(nart_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 2) return NART_E_INVALID;
    ctx->specialize = mode != 0;
    ctx->lean = mode == 2;
    for (nart_ctx* c : ctx->subs) {
        c->specialize = ctx->specialize;
        c->lean = ctx->lean;
    }
    return NART_OK;
}

int nart_hip_scene_features_of(const nart_scene_blob* scene, uint32_t* features) {
    if (!scene || !features) return NART_E_INVALID;
    *features = scene_features(scene);
    return NART_OK;
}

int nart_hip_scene_features(const nart_ctx* ctx, uint32_t* features, uint32_t* build) {
    if (!ctx) return NART_E_INVALID;
    const nart_ctx* c = first_device(ctx);
    if (features) *features = c->features;
    if (build) *build = c->fm_used;
    return NART_OK;
}

int nart_hip_set_variant(nart_ctx* ctx, int variant) {
    if (!ctx) return NART_E_INVALID;
    for (nart_ctx* c : ctx->subs)
        if (int rc = nart_hip_set_variant(c, variant)) return fail(ctx, rc, c->err);
    if (variant != 0 && variant != 3)
        return fail(ctx, NART_E_UNSUPPORTED, "variant must be 0 (megakernel with a wave ray queue) or 3 (megakernel, "
                                             "one lane per pixel); the wavefront variant 1 and the traversal-quorum "
                                             "variant 2 were retired (DESIGN.md)");
    ctx->variant = variant;
    return NART_OK;
}

int nart_hip_render_buckets_async(nart_ctx* ctx, const nart_render_params* p, const uint32_t* bucket_ids,
                                  uint32_t n_buckets, nart_pixel* d_tiles, void* stream, nart_render_stats* stats) {
    if (!ctx || !bucket_ids || !d_tiles) return NART_E_INVALID;
    if (!ctx->subs.empty())
        return fail(ctx, NART_E_UNSUPPORTED, "render_buckets_async takes a single-device context (one per rank)");
    RenderTimer timer(stats);
    if (int rc = check_params(ctx, p)) return rc;
    const FrameTiles out(plan_frame(FrameAsk(p->integrator), PlanRules::Buckets), reinterpret_cast<float*>(d_tiles), 0);
    return render_buckets(ctx, p, bucket_ids, n_buckets, out, (hipStream_t)stream, stats);
}

int nart_hip_combine_async(nart_ctx* ctx, const nart_render_params* p, const nart_pixel* d_tiles, nart_pixel* d_image,
                           void* stream) {
    if (!ctx || !p || !d_tiles || !d_image) return NART_E_INVALID;
    if (!ctx->subs.empty()) return nart_hip_combine_async(first_device(ctx), p, d_tiles, d_image, stream);
    HIPCHK(hipSetDevice(ctx->device));
    const ImageLayout layout(p);
    const nart_session_geometry& g = layout.g;
    CombineArgs ca;
    ca.tiles = reinterpret_cast<const float*>(d_tiles);
    ca.image = reinterpret_cast<float*>(d_image);
    layout.fill(ca);
    ca.B = p->bucket_size;
    ca.tile = g.tile_size;
    ca.nbx = g.n_buckets_x;
    ca.nby = g.n_buckets_y;
    uint64_t n = (uint64_t)g.total_width * g.total_height;
    hipLaunchKernelGGL(k_combine, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ca);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

int nart_hip_render(nart_ctx* ctx, const nart_render_params* p, nart_pixel* image, nart_render_stats* stats) {
    if (!ctx || !p || !image) return NART_E_INVALID;
    const FramePlan plan = plan_frame(FrameAsk(p->integrator), PlanRules::Frame);
    FrameRequest rq;
    rq.to_host(plan, OutputKind::Beauty, image);
    return render_frame(ctx, p, plan, rq, stats);
}

int nart_hip_render_aovs(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, nart_pixel* image,
                         nart_pixel* albedo, nart_pixel* normal, nart_render_stats* stats, double* aov_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    if (!aovs && !image) return fail(ctx, NART_E_INVALID, "neither the beauty nor an AOV is requested");
    if (!aovs) return nart_hip_render(ctx, p, image, stats);
    return render_aovs(ctx, p, nullptr, aovs, image, albedo, normal, nullptr, stats, aov_ms, nullptr);
}

int nart_hip_render_moment(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, nart_pixel* image,
                           nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment, nart_render_stats* stats,
                           double* aov_ms, double* moment_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    if (!moment) return fail(ctx, NART_E_INVALID, "the moment image buffer is required");
    return render_aovs(ctx, p, nullptr, aovs, image, albedo, normal, moment, stats, aov_ms, moment_ms);
}

int nart_hip_render_halves(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, const nart_guide_params* gp,
                           nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* half_a, nart_pixel* half_b,
                           nart_render_stats* stats, double* halves_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    nart_guide_params g;
    if (gp)
        if (const char* why = guide_params_error(gp, g)) return fail(ctx, NART_E_INVALID, why);
    return render_halves(ctx, p, gp ? &g : nullptr, aovs, image, albedo, normal, half_a, half_b, stats, halves_ms);
}

void nart_hip_adaptive_params_init(nart_adaptive_params* ap) {
    if (ap) *ap = ADAPTIVE_DEFAULTS;
}

int nart_hip_adaptive_levels(const nart_adaptive_params* ap, uint32_t spp, uint32_t* levels, uint32_t* n) {
    if (!n) return NART_E_INVALID;
    nart_adaptive_params a;
    if (adaptive_params_error(ap, a, spp)) return NART_E_INVALID;
    const std::vector<uint32_t> l = adaptive_levels(a, spp);
    *n = (uint32_t)l.size();
    if (levels) std::copy(l.begin(), l.end(), levels);
    return NART_OK;
}

int nart_hip_render_adaptive(nart_ctx* ctx, const nart_render_params* p, const nart_adaptive_params* ap, uint32_t aovs,
                             nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment,
                             uint32_t* bucket_spp, float* bucket_error, nart_render_stats* stats, double* adaptive_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    if (adaptive_ms) *adaptive_ms = 0.0;
    if (const char* why = aov_request_error(aovs, albedo, normal)) return fail(ctx, NART_E_INVALID, why);
    AdaptiveRun run;
    if (const char* why = adaptive_params_error(ap, run.ap, p->spp)) return fail(ctx, NART_E_INVALID, why);
    run.levels = adaptive_levels(run.ap, p->spp);
    FrameAsk ask(p->integrator);
    ask.adaptive = true;
    ask.moment = moment != nullptr;
    ask_aovs(ask, aovs);
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    FrameRequest rq;
    rq.adaptive = &run;
    aovs_to_host(rq, plan, false, image, albedo, normal, moment);
    if (int rc = render_frame(ctx, p, plan, rq, stats)) return rc;
    if (bucket_spp) std::copy(run.spp.begin(), run.spp.end(), bucket_spp);
    if (bucket_error) std::copy(run.err.begin(), run.err.end(), bucket_error);
    if (adaptive_ms) *adaptive_ms = run.ms;
    return NART_OK;
}

void nart_hip_cascade_defaults(nart_cascade_params* cp) {
    if (cp) *cp = CASCADE_DEFAULTS;
}

int nart_hip_cascade_levels(const nart_cascade_params* cp, float* levels, uint32_t* n) {
    if (!n) return NART_E_INVALID;
    nart_cascade_params c;
    CascadeLevels lv;
    if (cascade_params_error(cp, c, lv)) return NART_E_INVALID;
    *n = lv.K;
    if (levels) std::copy(lv.b, lv.b + lv.K, levels);
    return NART_OK;
}

int nart_hip_render_cascade(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params* cp, nart_pixel* image,
                            nart_pixel* beauty, nart_pixel* layers, nart_render_stats* stats) {
    nart_cascade_params c;
    CascadeLevels lv;
    if (const char* why = cascade_params_error(cp, c, lv)) return fail(ctx, NART_E_INVALID, why);
    if (!ctx || !p || !image) return NART_E_INVALID;
    if (const char* why = check_cascade_frame(p)) return fail(ctx, NART_E_INVALID, why);
    return render_cascade(ctx, p, c, lv, image, beauty, layers, stats);
}

int nart_hip_cascade_reweight(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params* cp,
                              const nart_pixel* beauty, const nart_pixel* layers, nart_pixel* image) {
    nart_cascade_params c;
    CascadeLevels lv;
    if (const char* why = cascade_params_error(cp, c, lv)) return fail(ctx, NART_E_INVALID, why);
    if (!ctx || !p || !beauty || !layers || !image) return NART_E_INVALID;
    if (const char* why = check_cascade_frame(p)) return fail(ctx, NART_E_INVALID, why);
    return cascade_host(ctx, p, c, lv, beauty, layers, image);
}

int nart_hip_cascade_timings(const nart_ctx* ctx, double* cascade_ms, double* reweight_ms) {
    if (!ctx) return NART_E_INVALID;
    if (cascade_ms) *cascade_ms = ctx->cas_ms[0];
    if (reweight_ms) *reweight_ms = first_device(ctx)->cas_ms[1];
    return NART_OK;
}

void nart_hip_matte_defaults(nart_matte_params* mp) {
    if (mp) *mp = MATTE_DEFAULTS;
}

int nart_hip_matte_ids(const nart_scene_blob* scene, uint32_t kind, uint32_t* n_ids) {
    if (!scene || !n_ids || (kind != NART_MATTE_MESH && kind != NART_MATTE_MATERIAL)) return NART_E_INVALID;
    *n_ids = kind == NART_MATTE_MATERIAL ? scene->num_materials : scene->num_meshes;
    return *n_ids > MATTE_MAX_IDS ? NART_E_UNSUPPORTED : NART_OK;
}

int nart_hip_render_mattes(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp, nart_pixel* ranks,
                           nart_pixel* image, nart_pixel* planes, nart_render_stats* stats) {
    nart_matte_params m;
    if (const char* why = matte_params_error(mp, m)) return fail(ctx, NART_E_INVALID, why);
    if (!ctx || !p || !ranks) return NART_E_INVALID;
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return render_mattes(ctx, p, m, ranks, image, planes, stats);
}

int nart_hip_matte_rank(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp, uint32_t n_ids,
                        const nart_pixel* planes, nart_pixel* ranks) {
    nart_matte_params m;
    if (const char* why = matte_params_error(mp, m)) return fail(ctx, NART_E_INVALID, why);
    if (n_ids > MATTE_MAX_IDS) return fail(ctx, NART_E_INVALID, "n_ids must be <= 32");
    if (!ctx || !p || !ranks || (n_ids && !planes)) return NART_E_INVALID;
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return matte_rank_host(ctx, p, m, n_ids, planes, ranks);
}

int nart_hip_matte_extract(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp, const nart_pixel* ranks,
                           uint64_t id_mask, nart_pixel* out) {
    nart_matte_params m;
    if (const char* why = matte_params_error(mp, m)) return fail(ctx, NART_E_INVALID, why);
    if (!ctx || !p || !ranks || !out) return NART_E_INVALID;
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return matte_extract_host(ctx, p, m, ranks, id_mask, out);
}

int nart_hip_matte_timings(const nart_ctx* ctx, double* matte_ms, double* rank_ms) {
    if (!ctx) return NART_E_INVALID;
    if (matte_ms) *matte_ms = ctx->mat_ms[0];
    if (rank_ms) *rank_ms = first_device(ctx)->mat_ms[1];
    return NART_OK;
}

int nart_hip_render_light_groups(nart_ctx* ctx, const nart_render_params* p, const uint32_t* group_of_light,
                                 uint32_t n_lights, uint32_t n_groups, nart_pixel* groups, nart_pixel* image,
                                 nart_render_stats* stats) {
    if (!ctx || !p || !groups) return NART_E_INVALID;
    if (const char* why = light_groups_error(group_of_light, n_lights, first_device(ctx)->scene.num_lights, n_groups))
        return fail(ctx, NART_E_INVALID, why);
    return render_light_groups(ctx, p, group_of_light, n_groups, groups, image, stats);
}

int nart_hip_light_mix(nart_ctx* ctx, const nart_render_params* p, uint32_t n_groups, const float* gains,
                       const nart_pixel* groups, nart_pixel* out) {
    if (!ctx || !p) return NART_E_INVALID;
    if (const char* why = light_mix_error(n_groups, gains, groups, out)) return fail(ctx, NART_E_INVALID, why);
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return light_mix_host(ctx, p, n_groups, gains, groups, out);
}

int nart_hip_render_light_group_samples(nart_ctx* ctx, const nart_render_params* p, const uint32_t* group_of_light,
                                        uint32_t n_lights, uint32_t n_groups, uint32_t x0, uint32_t y0, uint32_t w,
                                        uint32_t h, float* out) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_light_group_samples(first_device(ctx), p, group_of_light, n_lights, n_groups,
                                                                  x0, y0, w, h, out));
    if (const char* why = light_groups_error(group_of_light, n_lights, ctx->scene.num_lights, n_groups))
        return fail(ctx, NART_E_INVALID, why);
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->integrator == NART_INTEGRATOR_VOLUME)  // (frames: plan_frame's rule)
        return fail(ctx, NART_E_UNSUPPORTED, "light groups need the path integrator: the volume integrator has no light-group build");
    if (!w || !h) return fail(ctx, NART_E_INVALID, "empty rect");
    if ((rc = set_light_groups(ctx, group_of_light)) || (rc = counter_buffer(ctx))) return rc;
    RenderArgs ra;
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, ctx->d_counters.as<unsigned long long>(), ra))) return rc;
    const size_t ns = (size_t)ra.n_slots * p->spp;
    Buf records;  // the G record arrays; freed on return
    if ((rc = reserve(ctx, records, ctx->device, n_groups * ns * sizeof(float4), "light-group records"))) return rc;
    HIPCHK(hipMemsetAsync(records.as<void>(), 0, n_groups * ns * sizeof(float4), 0));
    ra.n_groups = n_groups;
    ra.light_group = ctx->d_light_group.as<uint32_t>();
    ra.Lgrp = records.as<float4>();
    ra.lgrp_stride = ns;
    if ((rc = launch_latin(ctx, ra, 0)) || (rc = dispatch_render(ctx, ra, p->integrator, 0))) return rc;
    HIPCHK(hipMemcpy(out, records.as<float4>(), n_groups * ns * sizeof(float4), hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_light_group_timings(const nart_ctx* ctx, double* splat_ms, double* mix_ms) {
    if (!ctx) return NART_E_INVALID;
    if (splat_ms) *splat_ms = ctx->lg_ms[0];
    if (mix_ms) *mix_ms = first_device(ctx)->lg_ms[1];
    return NART_OK;
}

int nart_hip_render_depth_cuts(nart_ctx* ctx, const nart_render_params* p, const uint32_t* cuts, uint32_t n_cuts,
                               nart_pixel* cut_images, nart_pixel* image, nart_render_stats* stats) {
    if (!ctx || !p || !cut_images) return NART_E_INVALID;
    if (const char* why = depth_cuts_error(cuts, n_cuts, p->bounces)) return fail(ctx, NART_E_INVALID, why);
    return render_depth_cuts(ctx, p, cuts, n_cuts, cut_images, image, stats);
}

int nart_hip_depth_layers(nart_ctx* ctx, const nart_render_params* p, uint32_t n_cuts, const nart_pixel* cut_images,
                          const nart_pixel* beauty, nart_pixel* out) {
    if (!ctx || !p) return NART_E_INVALID;
    if (n_cuts < 1 || n_cuts > NART_DEPTH_CUTS_MAX) return fail(ctx, NART_E_INVALID, "n_cuts must be 1..8");
    if (!cut_images || !beauty || !out) return fail(ctx, NART_E_INVALID, "the cut images, the beauty and the layers are required");
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return depth_layers_host(ctx, p, n_cuts, cut_images, beauty, out);
}

int nart_hip_render_depth_cut_samples(nart_ctx* ctx, const nart_render_params* p, const uint32_t* cuts, uint32_t n_cuts,
                                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float* out) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_depth_cut_samples(first_device(ctx), p, cuts, n_cuts, x0, y0, w, h, out));
    if (const char* why = depth_cuts_error(cuts, n_cuts, p->bounces)) return fail(ctx, NART_E_INVALID, why);
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->integrator == NART_INTEGRATOR_VOLUME)  // (frames: plan_frame's rule)
        return fail(ctx, NART_E_UNSUPPORTED, "depth cuts need the path integrator: the volume integrator has no depth-cut build");
    if (!w || !h) return fail(ctx, NART_E_INVALID, "empty rect");
    if ((rc = counter_buffer(ctx))) return rc;
    RenderArgs ra;
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, ctx->d_counters.as<unsigned long long>(), ra))) return rc;
    const size_t ns = (size_t)ra.n_slots * p->spp;
    Buf records;  // the K record arrays; freed on return
    if ((rc = reserve(ctx, records, ctx->device, n_cuts * ns * sizeof(float4), "depth-cut records"))) return rc;
    ra.n_groups = n_cuts;
    for (uint32_t j = 0; j < n_cuts; ++j) ra.cuts[j] = cuts[j];
    ra.Lgrp = records.as<float4>();
    ra.lgrp_stride = ns;
    if ((rc = launch_latin(ctx, ra, 0)) || (rc = dispatch_render(ctx, ra, p->integrator, 0))) return rc;
    HIPCHK(hipMemcpy(out, records.as<float4>(), n_cuts * ns * sizeof(float4), hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_depth_cut_timings(const nart_ctx* ctx, double* splat_ms, double* layers_ms) {
    if (!ctx) return NART_E_INVALID;
    if (splat_ms) *splat_ms = ctx->dc_ms[0];
    if (layers_ms) *layers_ms = first_device(ctx)->dc_ms[1];
    return NART_OK;
}

int nart_hip_cost_grid(const nart_render_params* p, uint32_t* width, uint32_t* height) {
    if (!p || !width || !height) return NART_E_INVALID;
    if (check_image_size(p) || !p->bucket_size) return NART_E_INVALID;
    cost_grid_of(p, width, height);
    return NART_OK;
}

int nart_hip_render_cost(nart_ctx* ctx, const nart_render_params* p, nart_cost_pixel* cost, nart_pixel* beauty,
                         nart_render_stats* stats) {
    if (!ctx || !p) return NART_E_INVALID;
    if (!cost) return fail(ctx, NART_E_INVALID, "the cost grid is required");
    return render_cost(ctx, p, cost, beauty, stats);
}

int nart_hip_render_cost_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w,
                                 uint32_t h, uint32_t* records) {
    if (!ctx || !p || !records) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_cost_samples(first_device(ctx), p, x0, y0, w, h, records));
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->integrator == NART_INTEGRATOR_VOLUME)  // (frames: plan_frame's rule)
        return fail(ctx, NART_E_UNSUPPORTED, "the cost image needs the path integrator: the volume integrator has no cost build");
    if (!w || !h) return fail(ctx, NART_E_INVALID, "empty rect");
    if ((rc = counter_buffer(ctx))) return rc;
    RenderArgs ra;
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, ctx->d_counters.as<unsigned long long>(), ra))) return rc;
    const size_t ns = (size_t)ra.n_slots * p->spp;
    Buf rec;  // the record array; freed on return
    if ((rc = reserve(ctx, rec, ctx->device, ns * sizeof(uint4), "cost records"))) return rc;
    ra.cost_rec = rec.as<uint4>();
    if ((rc = launch_latin(ctx, ra, 0)) || (rc = dispatch_render(ctx, ra, p->integrator, 0))) return rc;
    HIPCHK(hipMemcpy(records, rec.as<uint4>(), ns * sizeof(uint4), hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_cost_image(nart_ctx* ctx, const nart_render_params* p, const nart_cost_pixel* cost, nart_pixel* image) {
    if (!ctx || !p) return NART_E_INVALID;
    if (!cost || !image) return fail(ctx, NART_E_INVALID, "the cost grid and the image are required");
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    return cost_image_host(ctx, p, cost, image);
}

int nart_hip_cost_timings(nart_ctx* ctx, double* reduce_ms, double* image_ms) {
    if (!ctx) return NART_E_INVALID;
    if (reduce_ms) *reduce_ms = ctx->cost_ms[0];
    if (image_ms) *image_ms = first_device(ctx)->cost_ms[1];
    return NART_OK;
}

int nart_hip_render_aov_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w,
                                uint32_t h, float* out8, uint32_t* tri) {
    if (!ctx || !p || !out8) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_aov_samples(first_device(ctx), p, x0, y0, w, h, out8, tri));
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->integrator == NART_INTEGRATOR_VOLUME)  // (frames: plan_frame's rule)
        return fail(ctx, NART_E_UNSUPPORTED, "first-hit AOVs need surfaces: the volume integrator has none");
    if (!w || !h) return fail(ctx, NART_E_INVALID, "empty rect");  // (nart_hip_render_samples launches over it)
    RenderArgs ra;
    // k_primary<false, ...> and k_aov count nothing
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, nullptr, ra))) return rc;
    if ((rc = launch_latin(ctx, ra, 0)) || (rc = launch_aov_primary(ctx, ra, 0))) return rc;
    const size_t ns = (size_t)ra.n_slots * p->spp;
    std::vector<float> rec(ns * 4);
    for (int k = 0; k < 2; ++k) {
        if ((rc = launch_aov(ctx, ra, k, ctx->d_L.as<float4>(), 0))) return rc;
        HIPCHK(hipMemcpy(rec.data(), ctx->d_L.as<float4>(), ns * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ns; ++i) std::memcpy(out8 + i * 8 + 4 * k, rec.data() + i * 4, 4 * sizeof(float));
    }
    if (tri) HIPCHK(hipMemcpy(tri, ctx->d_prim.as<uint32_t>(), ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NART_OK;
}

void nart_hip_guide_defaults(nart_guide_params* gp) {
    if (gp) *gp = GUIDE_DEFAULTS;
}

int nart_hip_render_guides(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* gp, uint32_t aovs,
                           nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment,
                           nart_render_stats* stats, double* guide_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    nart_guide_params g;
    if (const char* why = guide_params_error(gp, g)) return fail(ctx, NART_E_INVALID, why);
    if (!aovs && !image && !moment) return fail(ctx, NART_E_INVALID, "neither the beauty, the moment image nor a guide is requested");
    return render_aovs(ctx, p, &g, aovs, image, albedo, normal, moment, stats, guide_ms, nullptr);
}

int nart_hip_render_denoised_guides(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                    const nart_guide_params* gp, int sample_variance, nart_pixel* image,
                                    nart_pixel* out, nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    nart_guide_params g;
    if (const char* why = guide_params_error(gp, g)) return fail(ctx, NART_E_INVALID, why);
    return render_denoised(ctx, p, dp, sample_variance != 0, image, out, stats, denoise_ms, &g);
}

int nart_hip_render_guide_samples(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* gp, uint32_t x0,
                                  uint32_t y0, uint32_t w, uint32_t h, float* out8, float* seg8, uint32_t* tri,
                                  uint32_t* n_seg) {
    if (!ctx || !p || !out8) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_guide_samples(first_device(ctx), p, gp, x0, y0, w, h, out8, seg8, tri, n_seg));
    nart_guide_params g;
    if (const char* why = guide_params_error(gp, g)) return fail(ctx, NART_E_INVALID, why);
    int rc = check_params(ctx, p);
    if (rc) return rc;
    if (p->integrator == NART_INTEGRATOR_VOLUME)  // (frames: plan_frame's rule)
        return fail(ctx, NART_E_UNSUPPORTED, "followed guides need surfaces: the volume integrator has none");
    if (!w || !h) return fail(ctx, NART_E_INVALID, "empty rect");
    RenderArgs ra;
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, nullptr, ra)) || (rc = launch_latin(ctx, ra, 0))) return rc;
    const size_t ns = (size_t)ra.n_slots * p->spp, M = g.max_follow + 1;
    // the normal records, the segments, their triangles and the counts: temporaries, freed on return
    Buf d_normal, d_seg, d_tri, d_n;
    if ((rc = reserve(ctx, d_normal, ctx->device, ns * sizeof(float4), "guide normal records")) ||
        (rc = reserve(ctx, d_seg, ctx->device, ns * M * 8 * sizeof(float), "guide segments")) ||
        (rc = reserve(ctx, d_tri, ctx->device, ns * M * sizeof(uint32_t), "guide segment triangles")) ||
        (rc = reserve(ctx, d_n, ctx->device, ns * sizeof(uint32_t), "guide segment counts")))
        return rc;
    GuideArgs ga;
    ga.albedo = ctx->d_L.as<float4>();
    ga.normal = d_normal.as<float4>();
    ga.max_follow = g.max_follow;
    ga.seg8 = d_seg.as<float>();
    ga.tri = d_tri.as<uint32_t>();
    ga.n_seg = d_n.as<uint32_t>();
    if ((rc = launch_guide<true>(ctx, ra, ga, 0))) return rc;
    std::vector<float> rec(ns * 4);
    for (int k = 0; k < 2; ++k) {
        HIPCHK(hipMemcpy(rec.data(), k ? ga.normal : ga.albedo, ns * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < ns; ++i) std::memcpy(out8 + i * 8 + 4 * k, rec.data() + i * 4, 4 * sizeof(float));
    }
    if (seg8) HIPCHK(hipMemcpy(seg8, ga.seg8, ns * M * 8 * sizeof(float), hipMemcpyDeviceToHost));
    if (tri) HIPCHK(hipMemcpy(tri, ga.tri, ns * M * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_seg) HIPCHK(hipMemcpy(n_seg, ga.n_seg, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return NART_OK;
}

void nart_hip_denoise_params_init(nart_denoise_params* dp) {
    if (dp) *dp = DENOISE_DEFAULTS;
}

int nart_hip_denoise(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, const nart_pixel* beauty,
                     const nart_pixel* albedo, const nart_pixel* normal, nart_pixel* out, double* denoise_ms) {
    if (!ctx || !p || !beauty || !albedo || !normal || !out) return NART_E_INVALID;
    return denoise_host(ctx, p, dp, beauty, albedo, normal, nullptr, out, denoise_ms);
}

int nart_hip_denoise_moment(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                            const nart_pixel* beauty, const nart_pixel* albedo, const nart_pixel* normal,
                            const nart_pixel* moment, nart_pixel* out, double* denoise_ms) {
    if (!ctx || !p || !beauty || !albedo || !normal || !moment || !out) return NART_E_INVALID;
    return denoise_host(ctx, p, dp, beauty, albedo, normal, moment, out, denoise_ms);
}

int nart_hip_render_denoised(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, nart_pixel* image,
                             nart_pixel* out, nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    return render_denoised(ctx, p, dp, false, image, out, stats, denoise_ms);
}

int nart_hip_render_denoised_moment(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                    nart_pixel* image, nart_pixel* out, nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    return render_denoised(ctx, p, dp, true, image, out, stats, denoise_ms);
}

int nart_hip_denoise_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                             double* finalize_ms) {
    if (!ctx) return NART_E_INVALID;
    denoise_times(first_device(ctx)->dn, prepare_ms, variance_ms, pass_ms, finalize_ms);
    return NART_OK;
}

int nart_hip_denoise_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, const nart_pixel* half_a,
                           const nart_pixel* half_b, const nart_pixel* beauty, const nart_pixel* albedo,
                           const nart_pixel* normal, nart_pixel* out, nart_pixel* error, double* denoise_ms) {
    if (!ctx || !p || !half_a || !half_b || !beauty || !albedo || !normal || !out) return NART_E_INVALID;
    return denoise_cross_host(ctx, p, dp, half_a, half_b, beauty, albedo, normal, out, error, denoise_ms);
}

int nart_hip_render_denoised_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                   const nart_guide_params* gp, nart_pixel* out, nart_pixel* error, nart_pixel* image,
                                   nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p || !out || !error) return NART_E_INVALID;
    nart_guide_params g;
    if (gp)
        if (const char* why = guide_params_error(gp, g)) return fail(ctx, NART_E_INVALID, why);
    return render_denoised_cross(ctx, p, dp, gp ? &g : nullptr, out, error, image, stats, denoise_ms);
}

int nart_hip_denoise_cross_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                                   double* finalize_ms) {
    if (!ctx) return NART_E_INVALID;
    denoise_times(first_device(ctx)->dnx, prepare_ms, variance_ms, pass_ms, finalize_ms);
    return NART_OK;
}

int nart_hip_denoise_parts(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, uint32_t n_parts,
                           const nart_pixel* parts, const nart_pixel* albedo, const nart_pixel* normal, nart_pixel* out,
                           nart_pixel* sum, double* denoise_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    nart_denoise_params d;
    nart_guide_params g;
    if (const char* why = denoise_parts_error(n_parts, parts && albedo && normal && out, dp, d, nullptr, g))
        return fail(ctx, NART_E_INVALID, why);
    return denoise_parts_host(ctx, p, d, n_parts, parts, albedo, normal, out, sum, denoise_ms);
}

int nart_hip_render_denoised_light_groups(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                          const nart_guide_params* gp, const uint32_t* group_of_light, uint32_t n_lights,
                                          uint32_t n_groups, nart_pixel* denoised, nart_pixel* sum, nart_pixel* groups,
                                          nart_pixel* image, nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    if (const char* why = light_groups_error(group_of_light, n_lights, first_device(ctx)->scene.num_lights, n_groups))
        return fail(ctx, NART_E_INVALID, why);
    nart_denoise_params d;
    nart_guide_params g;
    if (const char* why = denoise_parts_error(n_groups, denoised != nullptr, dp, d, gp, g)) return fail(ctx, NART_E_INVALID, why);
    ctx->lg_ms[0] = 0.0;
    FrameAsk ask(p->integrator);
    ask.light_groups = n_groups;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is uploaded)
    if (int rc = set_light_groups(ctx, group_of_light)) return rc;
    const int rc = render_denoised_parts(ctx, p, d, gp ? &g : nullptr, plan, 0, n_groups, denoised, sum, groups, image, stats,
                                         denoise_ms);
    for (const nart_ctx* c : ctx->subs) ctx->lg_ms[0] = std::max(ctx->lg_ms[0], c->lg_ms[0]);  // the slowest device's
    return rc;
}

int nart_hip_render_denoised_depth_layers(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                          const nart_guide_params* gp, const uint32_t* cuts, uint32_t n_cuts,
                                          nart_pixel* denoised, nart_pixel* sum, nart_pixel* layers, nart_pixel* image,
                                          nart_render_stats* stats, double* denoise_ms) {
    if (!ctx || !p) return NART_E_INVALID;
    if (const char* why = depth_cuts_error(cuts, n_cuts, p->bounces)) return fail(ctx, NART_E_INVALID, why);
    nart_denoise_params d;
    nart_guide_params g;
    if (const char* why = denoise_parts_error(n_cuts + 1, denoised != nullptr, dp, d, gp, g))
        return fail(ctx, NART_E_INVALID, why);
    ctx->dc_ms[0] = first_device(ctx)->dc_ms[1] = 0.0;
    FrameAsk ask(p->integrator);
    ask.depth_cuts = n_cuts;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);
    set_depth_cuts(ctx, cuts, n_cuts);
    const int rc = render_denoised_parts(ctx, p, d, gp ? &g : nullptr, plan, n_cuts, n_cuts + 1, denoised, sum, layers, image,
                                         stats, denoise_ms);
    for (const nart_ctx* c : ctx->subs) ctx->dc_ms[0] = std::max(ctx->dc_ms[0], c->dc_ms[0]);  // the slowest device's
    return rc;
}

int nart_hip_denoise_parts_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                                   double* finalize_ms, double* sum_ms, double* guides_ms) {
    if (!ctx) return NART_E_INVALID;
    const DenoiseTimes& t = first_device(ctx)->dnp;
    denoise_times(t, prepare_ms, variance_ms, pass_ms, finalize_ms);
    if (sum_ms) *sum_ms = t.ms[DN_SLOT_SUM];
    if (guides_ms) *guides_ms = ctx->dnp_guides_ms;
    return NART_OK;
}

int nart_hip_render_device(nart_ctx* ctx, const nart_render_params* p, const nart_pixel** d_image,
                           nart_render_stats* stats) {
    if (!ctx || !p || !d_image) return NART_E_INVALID;
    // tiles gathered to device 0 and combined there (a multi-device context), into the context's image
    const FrameRequest rq(&ctx->d_image, 0);
    if (int rc = render_frame(ctx, p, plan_frame(FrameAsk(p->integrator), PlanRules::Frame), rq, stats)) return rc;
    if (ctx->subs.empty()) {  // (a multi-device frame has waited for its gather stream)
        RenderTimer timer(stats);
        if (hipStreamSynchronize(0) != hipSuccess) return fail(ctx, NART_E_HIP, "render");
    }
    *d_image = ctx->d_image.as<const nart_pixel>();
    return NART_OK;
}

int nart_hip_render_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w,
                            uint32_t h, float* out) {
    if (!ctx || !p || !out) return NART_E_INVALID;
    if (!ctx->subs.empty())  // per-sample debugging runs on the first device
        return forwarded(ctx, nart_hip_render_samples(first_device(ctx), p, x0, y0, w, h, out));
    int rc = check_params(ctx, p);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    if ((rc = counter_buffer(ctx))) return rc;
    unsigned long long* const d_counters = ctx->d_counters.as<unsigned long long>();
    if (ctx->counters) HIPCHK(hipMemset(d_counters, 0, ctx->d_counters.bytes()));
    RenderArgs ra;
    if ((rc = rect_slots(ctx, p, x0, y0, w, h, d_counters, ra))) return rc;
    if ((rc = launch_latin(ctx, ra, 0)) || (rc = dispatch_render(ctx, ra, p->integrator, 0))) return rc;
    HIPCHK(hipMemcpy(out, ctx->d_L.as<float4>(), (size_t)ra.n_slots * p->spp * sizeof(float4), hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_bvh_info(const nart_scene_blob* blob, nart_bvh_info* out) {
    if (!blob || !out) return NART_E_INVALID;
    std::vector<uint8_t> mask;
    bool root_leaf = false;
    uint32_t n_chunks = 0;
    nart::reference_visibility(*blob, mask, root_leaf, n_chunks, nullptr);
    nart::BuiltBVH bvh;
    nart::build_bvh(*blob, mask, 0.f, bvh);
    out->num_nodes = (uint32_t)bvh.nodes.size();
    out->stack_depth = std::max<uint32_t>(bvh.max_stack + 1, 2);  // as nart_hip_create
    out->num_leaf_tris = bvh.num_leaf_tris;
    out->reserved = 0;
    return NART_OK;
}

int nart_hip_bvh_dump(const nart_scene_blob* blob, nart_bvh_dump_info* info, void* nodes, size_t nodes_cap,
                      float* tri_isect, size_t isect_cap, float* tri_perm, size_t perm_cap) {
    if (!blob || !info) return NART_E_INVALID;
    // as nart_hip_create's host build
    std::vector<uint8_t> mask;
    bool root_leaf = false;
    uint32_t n_chunks = 0;
    nart::RefOctree oct;
    nart::reference_visibility(*blob, mask, root_leaf, n_chunks, &oct);
    const float maxabs = scene_maxabs(*blob);
    const float pad = maxabs * 6.103515625e-05f + 1e-6f, margin = maxabs * 6.103515625e-05f;
    nart::BuiltBVH bvh;
    nart::build_bvh(*blob, mask, pad, bvh);
    nart::annotate_octree_leaves(*blob, oct, margin, bvh);
    info->num_nodes = (uint32_t)bvh.nodes.size();
    info->num_leaf_tris = (uint32_t)(bvh.tri_isect.size() / 16);
    info->stack_depth = std::max<uint32_t>(bvh.max_stack + 1, 2);
    info->root_code = bvh.root_code;
    info->pad = pad;
    info->on_device = 0;
    const int rc = bvh_dump_check(*info, nodes, nodes_cap, tri_isect, isect_cap, tri_perm, perm_cap);
    if (rc) return rc < 0 ? rc : NART_OK;
    std::vector<float> perm;
    permute_tri_records(bvh.tri_isect, perm);
    if (info->num_nodes) std::memcpy(nodes, bvh.nodes.data(), (size_t)info->num_nodes * sizeof(BVHNode));
    if (info->num_leaf_tris) {
        std::memcpy(tri_isect, bvh.tri_isect.data(), (size_t)info->num_leaf_tris * 64);
        std::memcpy(tri_perm, perm.data(), (size_t)info->num_leaf_tris * 3 * 64);
    }
    return NART_OK;
}

int nart_hip_context_bvh_dump(const nart_ctx* ctx, nart_bvh_dump_info* info, void* nodes, size_t nodes_cap,
                              float* tri_isect, size_t isect_cap, float* tri_perm, size_t perm_cap) {
    if (!ctx || !info) return NART_E_INVALID;
    const nart_ctx* c = first_device(ctx);
    info->num_nodes = c->num_nodes;
    info->num_leaf_tris = c->num_leaf_tris;
    info->stack_depth = c->stack_depth;
    info->root_code = c->root_code;
    info->pad = c->bvh_pad;
    info->on_device = c->bvh_on_device ? 1u : 0u;
    const int rc = bvh_dump_check(*info, nodes, nodes_cap, tri_isect, isect_cap, tri_perm, perm_cap);
    if (rc) return rc < 0 ? rc : NART_OK;
    if (hipSetDevice(c->device) != hipSuccess) return NART_E_HIP;
    const size_t nt = info->num_leaf_tris;
    if ((info->num_nodes &&
         hipMemcpy(nodes, c->d_nodes.as<void>(), (size_t)info->num_nodes * sizeof(BVHNode), hipMemcpyDeviceToHost) !=
             hipSuccess) ||
        (nt && (hipMemcpy(tri_isect, c->d_tri_isect.as<void>(), nt * 64, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(tri_perm, c->d_tri_perm.as<void>(), nt * 3 * 64, hipMemcpyDeviceToHost) != hipSuccess))) {
        (void)hipGetLastError();
        return NART_E_HIP;
    }
    return NART_OK;
}

int nart_hip_env_search(const float* v, uint32_t n, const float* values, uint32_t m, uint32_t* full,
                        uint32_t* guided) {
    if (!v || !values || !full || !guided || !n) return NART_E_INVALID;
    std::vector<uint32_t> g(NART_ENV_GUIDE_K);
    const bool ok = env_guide(v, n, g.data());
    for (uint32_t i = 0; i < m; ++i) {
        full[i] = binary_search(values[i], v, 0, n);
        guided[i] = guided_search(values[i], v, 0, n, ok ? g.data() : nullptr);
    }
    return ok ? 1 : 0;
}

int nart_hip_splat_lut(float filter_width, float* cells4, uint32_t* n_cells, uint32_t* b0) {
    if (!cells4 || !n_cells || !b0) return NART_E_INVALID;
    float table[64 + 65];
    nart_filter_table(table);
    std::vector<LutCell> lut;
    if (!splat_thresholds(filter_width, table + 64) || !splat_lut(table + 64, table, lut, *b0)) return NART_E_INVALID;
    std::memcpy(cells4, lut.data(), lut.size() * sizeof(LutCell));
    *n_cells = (uint32_t)lut.size();
    return NART_OK;
}

int nart_hip_splat_thresholds(float filter_width, float* thr65) {
    if (!thr65) return NART_E_INVALID;
    return splat_thresholds(filter_width, thr65) ? NART_OK : NART_E_INVALID;
}

int nart_hip_eval_sincos(nart_ctx* ctx, const float* x, uint32_t n, float* s, float* c) {
    if (!ctx || !x || !s || !c) return NART_E_INVALID;
    if (!ctx->subs.empty()) return nart_hip_eval_sincos(first_device(ctx), x, n, s, c);
    HIPCHK(hipSetDevice(ctx->device));
    Buf bx, bs, bc;  // freed on return
    int rc = NART_OK;
    for (Buf* b : {&bx, &bs, &bc})
        if ((rc = reserve(ctx, *b, ctx->device, (size_t)n * 4 + 4, "sincos values"))) return rc;
    float *const dx = bx.as<float>(), *const ds = bs.as<float>(), *const dc = bc.as<float>();
    HIPCHK(hipMemcpy(dx, x, (size_t)n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sincos, dim3((n + 255) / 256), dim3(256), 0, 0, dx, n, ds, dc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(s, ds, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(c, dc, (size_t)n * 4, hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_eval(nart_ctx* ctx, uint32_t op, uint32_t fm, const float* in, uint32_t n, float* out) {
    if (!ctx || !in || !out || op >= NART_EVAL_N_OPS || !probe_fm_ok(fm) || n > NART_EVAL_MAX_N) return NART_E_INVALID;
    if (!n) return NART_OK;
    if (!ctx->subs.empty()) return nart_hip_eval(first_device(ctx), op, fm, in, n, out);
    HIPCHK(hipSetDevice(ctx->device));
    Buf bi, bo;  // freed on return
    int rc = NART_OK;
    const size_t bytes = (size_t)n * NART_EVAL_WORDS * sizeof(float);
    for (Buf* b : {&bi, &bo})
        if ((rc = reserve(ctx, *b, ctx->device, bytes, "probe records"))) return rc;
    float *const di = bi.as<float>(), *const dout = bo.as<float>();
    HIPCHK(hipMemcpy(di, in, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe, dim3((n + 255) / 256), dim3(256), 0, 0, op, fm, di, n, dout);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_trace(nart_ctx* ctx, uint32_t variant, uint32_t sk, int count, const float* in, uint32_t n, uint32_t* out) {
    if (!ctx || !in || !out || variant >= NART_TRACE_N_VARIANTS || n > NART_EVAL_MAX_N) return NART_E_INVALID;
    if (!ctx->subs.empty()) return nart_hip_trace(first_device(ctx), variant, sk, count, in, n, out);
    const bool step = variant == NART_TRACE_STEP || variant == NART_TRACE_STEP_ROT;
    if (step && sk > ctx->stack_depth) return NART_E_INVALID;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t kind;
        std::memcpy(&kind, in + (size_t)i * NART_TRACE_IN_WORDS + 7, 4);
        if (kind > NART_TRACE_ANY || (kind == NART_TRACE_ANY && variant == NART_TRACE_PACKET)) return NART_E_INVALID;
    }
    if (!n) return NART_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Buf bi, bo, bg;  // freed on return
    int rc = NART_OK;
    const size_t bytes_in = (size_t)n * NART_TRACE_IN_WORDS * 4, bytes_out = (size_t)n * NART_TRACE_OUT_WORDS * 4;
    if ((rc = reserve(ctx, bi, ctx->device, bytes_in, "trace probe rays"))) return rc;
    if ((rc = reserve(ctx, bo, ctx->device, bytes_out, "trace probe records"))) return rc;
    const uint32_t depth = ctx->stack_depth, grid = (n + 255) / 256;
    TraceProbeArgs P;
    P.in = bi.as<float>();
    P.out = bo.as<uint32_t>();
    P.n = n;
    P.stack_depth = depth;
    // LDS as the render launch of the same entry point sizes it: the per-lane stack alone (k_guide,
    // k_primary), k_render's layout, a 256-lane ray-queue block's stack and staged nodes, the wave stacks
    size_t lds = (size_t)depth * 256 * 8;
    const void* kern = nullptr;
    if (variant == NART_TRACE_PLAIN || variant == NART_TRACE_LDS) {
        if (variant == NART_TRACE_LDS) {
            const LdsLayout l = k_render_layout(depth, ctx->num_nodes);
            P.lds_nodes = l.nodes;
            lds = l.bytes;
        }
        kern = count ? (const void*)k_trace_probe<true> : (const void*)k_trace_probe<false>;
    } else if (step) {
        const bool rot = variant == NART_TRACE_STEP_ROT, sh = sk != 0;
        const uint32_t lv = sh ? sk : depth;
        P.sk = lv;
        P.lds_nodes = staged_nodes(ctx->num_nodes, rq_lds_bytes(lv, 256), CU_LDS_BYTES);
        lds = (size_t)lv * 256 * 8 + node_lds_bytes(P.lds_nodes);
        if (sh && lv < depth) {
            if ((rc = reserve(ctx, bg, ctx->device, (size_t)grid * 256 * (depth - lv) * sizeof(int2), "trace probe stack columns")))
                return rc;
            P.gstack = bg.as<int2>();
        }
        const void* tab[2][2][2] = {
            {{(const void*)k_trace_probe_step<false, false, false>, (const void*)k_trace_probe_step<false, false, true>},
             {(const void*)k_trace_probe_step<false, true, false>, (const void*)k_trace_probe_step<false, true, true>}},
            {{(const void*)k_trace_probe_step<true, false, false>, (const void*)k_trace_probe_step<true, false, true>},
             {(const void*)k_trace_probe_step<true, true, false>, (const void*)k_trace_probe_step<true, true, true>}}};
        kern = tab[count ? 1 : 0][rot ? 1 : 0][sh ? 1 : 0];
    } else {
        lds = (size_t)depth * 4 * sizeof(uint4);
        kern = count ? (const void*)k_trace_probe_packet<true> : (const void*)k_trace_probe_packet<false>;
    }
    if (lds > (size_t)160 * 1024) return fail(ctx, NART_E_UNSUPPORTED, "trace probe LDS layout out of range");
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    HIPCHK(hipMemcpy(bi.as<float>(), in, bytes_in, hipMemcpyHostToDevice));
    void* args[] = {(void*)&ctx->scene, (void*)&P};
    HIPCHK(hipLaunchKernel(kern, dim3(grid), dim3(256), args, lds, 0));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, bo.as<uint32_t>(), bytes_out, hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_scene_eval(nart_ctx* ctx, uint32_t op, uint32_t build, const float* in, uint32_t n, float* out) {
    if (!ctx || !in || !out || op >= NART_SCENE_N_OPS || build >= NART_SCENE_N_BUILDS || n > NART_EVAL_MAX_N)
        return NART_E_INVALID;
    if (!ctx->subs.empty()) return forwarded(ctx, nart_hip_scene_eval(first_device(ctx), op, build, in, n, out));
    if (!scene_build_fits(build, ctx->features, ctx->has_env))
        return fail(ctx, NART_E_INVALID, "the scene does not fit the probe build's feature mask");
    const DMedium& med = ctx->scene.medium;
    const bool medium_op = op == NART_SCENE_DG_LOOKUP || op == NART_SCENE_MEDIUM_WALK;
    if (medium_op && !med.present) return fail(ctx, NART_E_INVALID, "the scene has no medium");
    // every index a record carries lies inside the scene, and no coordinate of a record can index outside
    // an environment distribution: the device functions check neither
    const bool light_op = op >= NART_SCENE_ENV_PDF && op <= NART_SCENE_LIGHT_SAMPLE_LI;
    for (uint32_t i = 0; i < n; ++i) {
        const float* x = in + (size_t)i * NART_SCENE_IN_WORDS;
        uint32_t idx;
        std::memcpy(&idx, x, 4);
        const uint32_t count = op == NART_SCENE_TEX_FETCH ? ctx->num_textures
                               : light_op                 ? ctx->scene.num_lights
                               : op == NART_SCENE_CREATE_BSDF ? ctx->num_materials
                                                              : 0xFFFFFFFFu;
        if (!medium_op && idx >= count) return fail(ctx, NART_E_INVALID, "a probe record's index is outside the scene");
        if (!light_op) continue;
        const DLight& L = ctx->lights[idx];
        const bool dist = L.type == NART_LIGHT_ENVIRONMENT && L.Le.type != NART_PTN_CONSTANT && L.env >= 0;
        if (op == NART_SCENE_ENV_PDF && L.type != NART_LIGHT_ENVIRONMENT)
            return fail(ctx, NART_E_INVALID, "ENV_PDF needs an environment light");
        if (op == NART_SCENE_ENV_PDF && dist) {
            const uint32_t w = ctx->env_dims[2 * (size_t)L.env], h = ctx->env_dims[2 * (size_t)L.env + 1];
            if (f2u32(gmin(x[1], 0.9999f) * (float)w) >= w || f2u32(gmin(x[2], 0.9999f) * (float)h) >= h)
                return fail(ctx, NART_E_INVALID, "an ENV_PDF record's coordinates index outside the distribution");
        }
        if (op == NART_SCENE_LIGHT_SAMPLE_LI && dist &&
            !(x[4] >= 0.f && x[4] <= 1.f && x[5] >= 0.f && x[5] <= 1.f))
            return fail(ctx, NART_E_INVALID, "a LIGHT_SAMPLE_LI record's sample is outside [0, 1]");
    }
    if (!n) return NART_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Buf bi, bo;  // freed on return
    int rc = NART_OK;
    const size_t bytes_in = (size_t)n * NART_SCENE_IN_WORDS * sizeof(float);
    const size_t bytes_out = (size_t)n * NART_SCENE_OUT_WORDS * sizeof(float);
    if ((rc = reserve(ctx, bi, ctx->device, bytes_in, "scene probe records"))) return rc;
    if ((rc = reserve(ctx, bo, ctx->device, bytes_out, "scene probe answers"))) return rc;
    SceneProbeArgs P;
    P.in = bi.as<float>();
    P.out = bo.as<float>();
    P.n = n;
    P.op = op;
    P.build = build;
    // the grid in LDS as dispatch_volume stages it
    if (op == NART_SCENE_DG_LOOKUP) P.lds_cells = volume_lds_cells(med.rx * med.ry * med.rz);
    HIPCHK(hipMemcpy(bi.as<float>(), in, bytes_in, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_scene_probe, dim3((n + 255) / 256), dim3(256), (size_t)P.lds_cells * sizeof(float), 0, ctx->scene, P);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, bo.as<float>(), bytes_out, hipMemcpyDeviceToHost));
    return NART_OK;
}

int nart_hip_context_bvh(const nart_ctx* ctx, nart_bvh_info* out, double* build_ms) {
    if (!ctx || !out) return NART_E_INVALID;
    const nart_ctx* c = first_device(ctx);
    out->num_nodes = c->num_nodes;
    out->stack_depth = c->stack_depth;
    out->num_leaf_tris = c->num_leaf_tris;
    out->reserved = c->bvh_on_device ? 1u : 0u;
    if (build_ms) *build_ms = c->bvh_ms;
    return NART_OK;
}

int nart_hip_device_count(int* count) {
    if (!count) return NART_E_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return NART_E_HIP;
    }
    *count = n;
    return NART_OK;
}

int nart_hip_shard_buckets(uint32_t n_buckets_x, uint32_t n_buckets, uint32_t n_devices, uint32_t device_index,
                           uint32_t* ids, uint32_t* count) {
    if (!count || !n_devices || !n_buckets_x || device_index >= n_devices) return NART_E_INVALID;
    const std::vector<uint32_t> v = shard_ids(n_buckets_x, n_buckets, n_devices, device_index);
    if (ids) std::memcpy(ids, v.data(), v.size() * sizeof(uint32_t));
    *count = (uint32_t)v.size();
    return NART_OK;
}

int nart_hip_create_multi(const nart_scene_blob* blob, const int* device_ids, int n_devices, nart_ctx** out) {
    if (!blob || !out || !device_ids || n_devices < 1 || n_devices > 64) return NART_E_INVALID;
    *out = nullptr;
    const char* gm = env_opt("NART_GATHER");
    const bool force_rccl = gm && std::string(gm) == "rccl";
    const bool force_copy = gm && std::string(gm) == "copy";
    if (n_devices == 1 && !force_rccl) return nart_hip_create(blob, device_ids[0], out);
    nart_ctx* ctx = new (std::nothrow) nart_ctx();
    if (!ctx) return NART_E_OOM;
    ctx->device = device_ids[0];
    auto bail = [&](int code) {
        nart_hip_destroy(ctx);
        return code;
    };
    bool distinct = true;
    for (int i = 0; i < n_devices; ++i)
        for (int j = 0; j < i; ++j) distinct = distinct && device_ids[i] != device_ids[j];
    for (int d = 0; d < n_devices; ++d) {
        nart_ctx* sub = nullptr;
        if (int rc = nart_hip_create(blob, device_ids[d], &sub)) return bail(rc);
        ctx->subs.push_back(sub);
        ctx->devs.push_back(device_ids[d]);
        ctx->sub_tiles.emplace_back();
        ctx->streams.emplace_back();
        ctx->streams.back().device = device_ids[d];
        if (hipSetDevice(device_ids[d]) != hipSuccess ||
            hipStreamCreateWithFlags(&ctx->streams.back().s, hipStreamNonBlocking) != hipSuccess)
            return bail(NART_E_HIP);
    }
    for (int d = 0; d < n_devices; ++d)
        for (int j = 0; j < n_devices; ++j) ctx->subs[d]->mem_share += (j != d && device_ids[j] == device_ids[d]) ? 1u : 0u;
    ctx->gather_rccl = force_rccl || (distinct && !force_copy);
    if (ctx->gather_rccl) {
        const RcclApi& R = rccl_api();
        bool ok = R.ok && distinct;
        if (ok) {
            ctx->comms.assign(n_devices, nullptr);
            if (R.CommInitAll(ctx->comms.data(), n_devices, device_ids) != ncclSuccess) {
                ctx->comms.clear();
                (void)hipGetLastError();
                ok = false;
            }
        }
        if (!ok) {
            // NART_GATHER=rccl demands RCCL; otherwise the device-copy gather serves the same
            // image (nart_hip_context_devices reports the fallback)
            if (force_rccl) return bail(NART_E_RCCL);
            ctx->gather_rccl = false;
            ctx->gather_fallback = true;
        }
    }
    if (!ctx->gather_rccl) {
        // device copies to device 0 (peer access where the devices differ)
        hipSetDevice(device_ids[0]);
        for (int d = 1; d < n_devices; ++d)
            if (device_ids[d] != device_ids[0]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, device_ids[0], device_ids[d]) == hipSuccess && can)
                    hipDeviceEnablePeerAccess(device_ids[d], 0);
                (void)hipGetLastError();  // already enabled is fine
            }
    }
    *out = ctx;
    return NART_OK;
}

int nart_hip_context_devices(const nart_ctx* ctx, int* n_devices, int* uses_rccl) {
    if (!ctx || !n_devices) return NART_E_INVALID;
    *n_devices = ctx->subs.empty() ? 1 : (int)ctx->subs.size();
    if (uses_rccl) *uses_rccl = ctx->gather_rccl ? 1 : (ctx->gather_fallback ? 2 : 0);
    return NART_OK;
}

int nart_hip_debug_fault(nart_ctx* ctx, int fault) {
    if (!ctx || fault < 0 || fault > 1) return NART_E_INVALID;
    ctx->debug_fault = fault;
    return NART_OK;
}

}  // extern "C"
