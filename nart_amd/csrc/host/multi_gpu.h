// Multi-GPU render context (nart_hip_create_multi), included by render.hip.
//
// The reference renders a session's buckets with a tbb::task_group over every host core and sums
// their tiles into the image in bucket raster order (render.cpp:152-203).  Here one process drives
// N GPUs of the node:
//   * the scene lives on every device (one single-device sub-context each, nart_hip_create);
//   * buckets are dealt over the devices on a diagonal lattice (shard_ids: every region of a frame
//     spreads evenly over all devices; nart_hip_shard_buckets);
//   * one host thread per device renders its share into device-resident tiles (render_buckets);
//   * the tiles are gathered to device 0 with one RCCL group of ncclSend / ncclRecv over xGMI
//     (library-owned communicator, ncclCommInitAll over the device list), permuted into bucket-id
//     order and combined in bucket raster order on device 0 (k_combine) -- so the image is
//     bit-identical for any N.
// An adaptive frame (FrameRequest::adaptive) differs in the third step only: each thread refines its
// device's share (render_buckets_adaptive) into the same slabs; gather and combine follow unchanged.
// RCCL is loaded at run time (dlopen), so single-device use never needs it.  A device list with
// repeated ordinals (a rehearsal of N ranks on fewer GPUs) gathers with device copies instead,
// since an RCCL communicator needs distinct GPUs.  NART_GATHER=rccl|copy overrides the choice
// (rccl on one device runs a self send/receive through RCCL).
#pragma once

#include <dlfcn.h>

#include <mutex>
#include <thread>

namespace {

struct RcclApi {
    bool ok = false;
    std::string err;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*ErrStr)(ncclResult_t) = nullptr;
};

const RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) {
            api.err = std::string("cannot load librccl: ") + dlerror();
            return;
        }
        bool all = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            all = all && fn;
        };
        sym(api.CommInitAll, "ncclCommInitAll");
        sym(api.CommDestroy, "ncclCommDestroy");
        sym(api.GroupStart, "ncclGroupStart");
        sym(api.GroupEnd, "ncclGroupEnd");
        sym(api.Send, "ncclSend");
        sym(api.Recv, "ncclRecv");
        sym(api.ErrStr, "ncclGetErrorString");
        api.ok = all;
        if (!all) api.err = "librccl lacks ncclCommInitAll/ncclSend/ncclRecv";
    });
    return api;
}

// Bucket ids of device d out of n, in ascending order: a diagonal lattice, bucket (bx, by) on
// device (bx + s*by) % n with s = lattice_step(n), the s in [1, n) coprime to n closest to 0.382 n.
// Every run of n buckets along a row or a column holds each device once, so every region of the
// frame -- the costly glass of C3 -- splits evenly over the devices.  (b % n gave whole vertical
// stripes when n divides the bucket-column count: C3 1/8 shards 86-101 ms.)  Must match
// nart_amd/dist.py bucket_owners.
uint32_t lattice_step(uint32_t n) {
    uint32_t best = 0;
    double bd = 1e30;
    for (uint32_t s = 1; s < n; ++s) {
        uint32_t a = s, b = n;
        while (b) {
            const uint32_t t = a % b;
            a = b;
            b = t;
        }
        const double dd = std::fabs((double)s - 0.382 * (double)n);
        if (a == 1 && dd < bd) {
            bd = dd;
            best = s;
        }
    }
    return best;
}

std::vector<uint32_t> shard_ids(uint32_t nbx, uint32_t n_buckets, uint32_t n, uint32_t d) {
    std::vector<uint32_t> ids;
    const uint32_t s = lattice_step(n);
    for (uint32_t b = 0; b < n_buckets; ++b)
        if ((uint32_t)(((uint64_t)(b % nbx) + (uint64_t)s * (b / nbx)) % n) == d) ids.push_back(b);
    return ids;
}

// Gathered slabs (device after device, each in its ascending id order) -> tiles in bucket-id
// order: slab tile i is bucket map[i].  One block per bucket.
__global__ void k_unshard(const float* slabs, float* by_id, const uint32_t* map, uint32_t n_buckets, uint32_t tile_floats) {
    const uint32_t i = blockIdx.x;
    if (i >= n_buckets) return;
    const float* src = slabs + (size_t)i * tile_floats;
    float* dst = by_id + (size_t)map[i] * tile_floats;
    for (uint32_t k = threadIdx.x; k < tile_floats; k += blockDim.x) dst[k] = src[k];
}

// The multi-device half of render_frame (which has validated p and sized a borrowed image buffer):
// shard, render concurrently, gather to device 0, combine, deliver.
// The gather runs over the plan's outputs.  Every device keeps their slabs back to back in
// sub_tiles[d] (slab i: output i), all are gathered in the one RCCL group (or by device copies), and
// each output is then permuted and combined into ctx->d_image on device 0 in turn, and copied to its
// destination (none where the request borrows ctx->d_image itself).  times: the slowest device's.
int render_multi(nart_ctx* ctx, const nart_render_params* p, const FramePlan& plan, const FrameRequest& rq,
                 nart_render_stats* stats, PassTimes& times) {
    const uint32_t n = (uint32_t)ctx->subs.size();
    const size_t K = plan.n_outputs;
    int rc = NART_OK;
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    const uint32_t nb = g.n_buckets_x * g.n_buckets_y;
    const size_t tile_floats = (size_t)g.tile_size * g.tile_size * 5;
    std::vector<std::vector<uint32_t>> ids(n);
    for (uint32_t d = 0; d < n; ++d) {
        ids[d] = shard_ids(g.n_buckets_x, nb, n, d);
        const size_t bytes = std::max<size_t>(1, ids[d].size()) * tile_floats * 4 * K;
        if ((rc = reserve(ctx, ctx->sub_tiles[d], ctx->devs[d], bytes, "device tiles"))) return rc;
    }
    const int dev0 = ctx->devs[0];
    const size_t all_bytes = (size_t)nb * tile_floats * 4;
    const size_t img_bytes = (size_t)g.total_width * g.total_height * sizeof(nart_pixel);
    if ((rc = reserve(ctx, ctx->d_gather, dev0, all_bytes * K, "gathered tiles")) ||
        (rc = reserve(ctx, ctx->d_byid, dev0, all_bytes, "tiles by bucket id")) ||
        (rc = reserve(ctx, ctx->d_image, dev0, img_bytes, "image")))
        return rc;
    HIPCHK(hipSetDevice(dev0));

    // 1. every device renders its buckets (one host thread each, like the TBB task group)
    std::vector<int> rcs(n, NART_OK);
    std::vector<nart_render_stats> st(n);
    std::vector<PassTimes> pass(n);
    std::vector<AdaptiveRun> runs;  // adaptive: one per device, parameters and levels copied in
    if (rq.adaptive) {
        runs.resize(n);
        for (AdaptiveRun& r : runs) {
            r.ap = rq.adaptive->ap;
            r.levels = rq.adaptive->levels;
        }
    }
    std::vector<std::thread> th;
    auto work = [&](uint32_t d) {
        if (ids[d].empty()) return;
        if (hipSetDevice(ctx->devs[d]) != hipSuccess) {
            rcs[d] = NART_E_HIP;
            return;
        }
        const FrameTiles out(plan, ctx->sub_tiles[d].as<float>(), ids[d].size() * tile_floats);
        if (rq.adaptive) {
            // the device refines its own shard: a bucket's error needs its own tiles only
            rcs[d] = render_buckets_adaptive(ctx->subs[d], p, ids[d].data(), (uint32_t)ids[d].size(), out,
                                             ctx->streams[d].s, &st[d], runs[d]);
            pass[d] = runs[d].passes;
        } else {
            rcs[d] = render_buckets(ctx->subs[d], p, ids[d].data(), (uint32_t)ids[d].size(), out, ctx->streams[d].s,
                                    &st[d], &pass[d]);
        }
        if (rcs[d] == NART_OK && hipStreamSynchronize(ctx->streams[d].s) != hipSuccess) rcs[d] = NART_E_HIP;
    };
    for (uint32_t d = 0; d < n; ++d) std::memset(&st[d], 0, sizeof(st[d]));
    try {
        th.reserve(n);
        for (uint32_t d = 0; d < n; ++d) th.emplace_back(work, d);
    } catch (...) {
        // no thread (or no room for one): join the ones started, report; nothing escapes the ABI
        for (auto& t : th) t.join();
        return fail(ctx, NART_E_OOM, "cannot start the per-device render threads");
    }
    for (auto& t : th) t.join();
    for (uint32_t d = 0; d < n; ++d)
        if (rcs[d] != NART_OK)
            return fail(ctx, rcs[d], "device " + std::to_string(ctx->devs[d]) + ": " + ctx->subs[d]->err);
    if (rq.adaptive) {
        // the shards' results in bucket-id order; buckets per level added up, the slowest device's time
        AdaptiveRun& out = *rq.adaptive;
        out.spp.assign(nb, 0);
        out.err.assign(nb, 0.f);
        out.rendered.assign(out.levels.size(), 0);
        for (uint32_t d = 0; d < n; ++d) {
            if (ids[d].empty()) continue;
            for (size_t i = 0; i < ids[d].size(); ++i) {
                out.spp[ids[d][i]] = runs[d].spp[i];
                out.err[ids[d][i]] = runs[d].err[i];
            }
            for (size_t l = 0; l < out.rendered.size(); ++l) out.rendered[l] += runs[d].rendered[l];
            out.ms = std::max(out.ms, runs[d].ms);
        }
    }

    // 2. gather the slabs to device 0 (rank order), RCCL over xGMI or device copies
    std::vector<size_t> first_b(n, 0);
    for (uint32_t d = 1; d < n; ++d) first_b[d] = first_b[d - 1] + ids[d - 1].size();
    float* slabs = ctx->d_gather.as<float>();
    hipStream_t s0 = ctx->streams[0].s;
    if (ctx->gather_rccl) {
        // every error inside the group is recorded and the group is always closed (an open group
        // would capture the next render's calls); a failed gather leaves the communicator in an
        // unknown state, so the context refuses further renders (rccl_broken)
        const RcclApi& R = rccl_api();
        ncclResult_t first = ncclSuccess;
        std::string where;
        auto note = [&](ncclResult_t r, const char* what) {
            if (r != ncclSuccess && first == ncclSuccess) {
                first = r;
                where = what;
            }
        };
        note(R.GroupStart(), "ncclGroupStart");
        if (first == ncclSuccess) {
            // test hook (nart_hip_debug_fault 1): the last device that owns buckets sends to a rank
            // that does not exist, after the receives of the devices before it are posted
            uint32_t last = n;
            for (uint32_t d = 0; d < n; ++d)
                if (!ids[d].empty()) last = d;
            const int bad_peer = ctx->debug_fault == 1 ? (int)n : 0;
            for (size_t i = 0; i < K; ++i)
                for (uint32_t d = 0; d < n; ++d) {
                    if (ids[d].empty()) continue;
                    const size_t cnt = ids[d].size() * tile_floats;
                    note(R.Send(ctx->sub_tiles[d].as<const float>() + i * cnt, cnt, ncclFloat32,
                                d == last ? bad_peer : 0, ctx->comms[d], ctx->streams[d].s),
                         "ncclSend");
                    note(R.Recv(slabs + (i * nb + first_b[d]) * tile_floats, cnt, ncclFloat32, (int)d, ctx->comms[0], s0),
                         "ncclRecv");
                }
            note(R.GroupEnd(), "ncclGroupEnd");
        }
        ctx->debug_fault = 0;
        if (first != ncclSuccess) {
            ctx->rccl_broken = true;
            for (uint32_t d = 0; d < n; ++d) {
                hipSetDevice(ctx->devs[d]);
                hipStreamSynchronize(ctx->streams[d].s);
            }
            (void)hipGetLastError();
            return fail(ctx, NART_E_RCCL, where + ": " + R.ErrStr(first) +
                                              " (context unusable: destroy it and create a new one)");
        }
        for (uint32_t d = 1; d < n; ++d) {
            HIPCHK(hipSetDevice(ctx->devs[d]));
            HIPCHK(hipStreamSynchronize(ctx->streams[d].s));
        }
        HIPCHK(hipSetDevice(dev0));
    } else {
        HIPCHK(hipSetDevice(dev0));
        for (size_t i = 0; i < K; ++i)
            for (uint32_t d = 0; d < n; ++d)
                if (!ids[d].empty())
                    HIPCHK(hipMemcpyPeerAsync(slabs + (i * nb + first_b[d]) * tile_floats, dev0,
                                              ctx->sub_tiles[d].as<const float>() + i * ids[d].size() * tile_floats,
                                              ctx->devs[d], ids[d].size() * tile_floats * 4, s0));
    }

    // 3. bucket-id order, raster-order combine on device 0, image to the host
    std::vector<uint32_t> map;
    map.reserve(nb);
    for (uint32_t d = 0; d < n; ++d) map.insert(map.end(), ids[d].begin(), ids[d].end());
    if ((rc = reserve(ctx, ctx->d_slab_map, dev0, (size_t)nb * 4, "slab map"))) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_slab_map.as<uint32_t>(), map.data(), (size_t)nb * 4, hipMemcpyHostToDevice, s0));
    // (stream order lets the buffers share d_byid and d_image)
    for (size_t i = 0; i < K; ++i) {
        if (!rq.on_device && !rq.dst[i]) continue;  // rendered for another output's sake, not delivered
        hipLaunchKernelGGL(k_unshard, dim3(nb), dim3(256), 0, s0, slabs + i * nb * tile_floats,
                           ctx->d_byid.as<float>(), ctx->d_slab_map.as<const uint32_t>(), nb,
                           (uint32_t)tile_floats);
        HIPCHK(hipGetLastError());
        if ((rc = nart_hip_combine_async(ctx->subs[0], p, ctx->d_byid.as<const nart_pixel>(),
                                         ctx->d_image.as<nart_pixel>(), s0)))
            return fail(ctx, rc, ctx->subs[0]->err);
        // output i: to its host image, or to image i of the borrowed device buffer
        void* dst = rq.on_device ? rq.image->as<char>() + i * img_bytes : static_cast<void*>(rq.dst[i]);
        if (dst != ctx->d_image.as<void>())
            HIPCHK(hipMemcpyAsync(dst, ctx->d_image.as<void>(), img_bytes,
                                  rq.on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s0));
    }
    HIPCHK(hipStreamSynchronize(s0));
    for (uint32_t d = 0; d < n; ++d)
        for (uint32_t k = 0; k < PASS_SLOTS; ++k) times.ms[k] = std::max(times.ms[k], pass[d].ms[k]);
    if (stats) {
        // one render: device times of the slowest device (they run concurrently), work counts
        // summed; added to the caller's stats as the single-device path adds a render's
        nart_render_stats m;
        std::memset(&m, 0, sizeof(m));
        for (uint32_t d = 0; d < n; ++d) add_stats(m, st[d], Times::Max);
        add_stats(*stats, m, Times::Sum);
    }
    return NART_OK;
}

}  // namespace
