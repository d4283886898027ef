// The stages over whole images that follow a frame -- the denoiser, the firefly cascade's reweighting,
// the ID mattes' ranking and extraction, the light groups' mix, the depth cuts' layers, the cost grid's
// image -- and the frames of the first-hit AOVs, the followed guides, the light groups, the depth cuts and
// the cost image; included by render.hip after render_frame.  Every stage has the same two layers:
//   X_device   its kernels over images of a view (Images, render.hip), named by their positions in it;
//   X_host     host images through the first device: upload, X_device, download (host_stage);
//   render_X   a frame into device images of the first device, X_device over them there, and what the
//              caller asked for to the host (frame_stage).
// The denoiser's images and work buffers are the context's, kept between calls; the cascade's and the
// mattes' images are temporaries of the call.  The parameters' rules are host/stage_params.h's.
// The parts denoise (light groups or depth layers denoised one by one with shared guides) is the one
// stage over two frames: the parts' frame and a guides frame, both into temporaries of the call.
#pragma once

namespace {

// Host images through device images of a single-device context: the inputs (k images each, where
// k may be 0) laid out back to back in `buf` from image 0, `stage` over the view, its n_out output
// images, which follow the inputs, to `out`.
struct HostImages {
    const nart_pixel* src;
    size_t k;
};
template <typename Stage>
int host_stage(nart_ctx* ctx, const nart_render_params* p, Buf& buf, const char* what,
               std::initializer_list<HostImages> in, nart_pixel* out, size_t n_out, Stage&& stage) {
    size_t n_in = 0;
    for (const HostImages& h : in) n_in += h.k;
    Images v(ctx, p);
    if (int rc = v.in(buf, n_in + n_out, what)) return rc;
    size_t i = 0;
    for (const HostImages& h : in) {
        if (int rc = v.upload(i, h.src, h.k)) return rc;
        i += h.k;
    }
    if (int rc = stage(v)) return rc;
    return v.download(n_in, out, n_out);
}

// The frame of `plan` into n_images device images in `buf` on the first device (the plan's outputs
// back to back in delivery order, room for the stage's after them), then `stage` over them on that
// device; render_ms covers the whole call.  A plan without outputs (the mattes of a scene without
// ids) renders nothing.  Errors of the first device are re-raised on ctx.
template <typename Stage>
int frame_stage(nart_ctx* ctx, const nart_render_params* p, const FramePlan& plan, Buf& buf, uint32_t n_images,
                nart_render_stats* stats, PassTimes* times, Stage&& stage) {
    nart_ctx* c0 = first_device(ctx);
    if (plan.code || plan.n_outputs) {
        if (int rc = render_frame(ctx, p, plan, FrameRequest(&buf, n_images), stats, times)) return rc;
    } else if (int rc = forwarded(ctx, check_params(c0, p))) {
        return rc;
    }
    RenderTimer timer(stats);
    Images v(c0, p);
    int rc = v.in(buf, n_images, "image");  // (sized by the frame: this lays them out)
    if (!rc) rc = stage(v);
    return forwarded(ctx, rc);
}

// ---------------------------------------------------------------- first-hit AOVs, followed guides
// The message of what is wrong with the AOV bits of a call and their image buffers, or null.
const char* aov_request_error(uint32_t aovs, const nart_pixel* albedo, const nart_pixel* normal, bool followed = false) {
    if (aovs & ~(NART_AOV_ALBEDO | NART_AOV_NORMAL)) return "unknown AOV bit";
    if (((aovs & NART_AOV_ALBEDO) && !albedo) || ((aovs & NART_AOV_NORMAL) && !normal))
        return followed ? "a guide is requested without its image buffer" : "an AOV is requested without its image buffer";
    return nullptr;
}

// The AOVs of `aovs` into the ask: first-hit, or with `follow` the followed guides in their place.
void ask_aovs(FrameAsk& ask, uint32_t aovs, const nart_guide_params* follow = nullptr) {
    bool* which = follow ? ask.guide : ask.aov;
    which[AOV_ALBEDO] = (aovs & NART_AOV_ALBEDO) != 0;
    which[AOV_NORMAL] = (aovs & NART_AOV_NORMAL) != 0;
    if (follow) ask.max_follow = follow->max_follow;
}

// Where the beauty, the two AOVs (or guides) and the moment image of `plan` go on the host.
void aovs_to_host(FrameRequest& rq, const FramePlan& plan, bool followed, nart_pixel* image, nart_pixel* albedo,
                  nart_pixel* normal, nart_pixel* moment) {
    rq.to_host(plan, OutputKind::Beauty, image);
    rq.to_host(plan, followed ? OutputKind::GuideAlbedo : OutputKind::Albedo, albedo);
    rq.to_host(plan, followed ? OutputKind::GuideNormal : OutputKind::Normal, normal);
    rq.to_host(plan, OutputKind::Moment, moment);
}

// nart_hip_render_aovs (moment null), nart_hip_render_moment and, with follow, nart_hip_render_guides:
// the followed guides in the first-hit AOVs' place.  aov_ms: the first-hit or the guide pass.
int render_aovs(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* follow, uint32_t aovs, nart_pixel* image,
                nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment, nart_render_stats* stats, double* aov_ms,
                double* moment_ms) {
    if (const char* why = aov_request_error(aovs, albedo, normal, follow != nullptr)) return fail(ctx, NART_E_INVALID, why);
    FrameAsk ask(p->integrator);
    // the moment image needs the path kernel: with it the beauty is rendered even where it is not asked for
    ask.beauty = image != nullptr || moment != nullptr;
    ask.moment = moment != nullptr;
    ask_aovs(ask, aovs, follow);
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    FrameRequest rq;
    aovs_to_host(rq, plan, follow != nullptr, image, albedo, normal, moment);
    PassTimes times;
    const int rc = render_frame(ctx, p, plan, rq, stats, &times);
    if (aov_ms) *aov_ms = times.ms[follow ? PASS_GUIDE : PASS_FIRST_HIT];
    if (moment_ms) *moment_ms = times.ms[PASS_MOMENT];
    return rc;
}

// The tile buffers a context keeps between whole frames grow with the number of outputs a frame
// has.  A cascade or matte frame has up to twelve, a half-buffer frame five: what it made them grow by is given back when the
// call returns, so that a later render finds the free memory (batch_slot_limit) it found before.
struct TileGrowthGuard {
    nart_ctx* ctx;
    size_t gather_bytes;
    std::vector<size_t> sub_bytes;
    explicit TileGrowthGuard(nart_ctx* c) : ctx(c), gather_bytes(c->d_gather.bytes()) {
        for (const Buf& b : c->sub_tiles) sub_bytes.push_back(b.bytes());
    }
    TileGrowthGuard(const TileGrowthGuard&) = delete;
    ~TileGrowthGuard() {
        if (ctx->d_gather.bytes() > gather_bytes) ctx->d_gather.release();
        for (size_t d = 0; d < sub_bytes.size(); ++d)
            if (ctx->sub_tiles[d].bytes() > sub_bytes[d]) ctx->sub_tiles[d].release();
    }
};

// ---------------------------------------------------------------- half buffers (device/halves.h)
// The ask of a half-buffer frame: the beauty, its two halves, and the AOVs of `aovs` (the followed
// guides with `follow`).
FrameAsk halves_ask(const nart_render_params* p, uint32_t aovs, const nart_guide_params* follow) {
    FrameAsk ask(p->integrator);
    ask.halves = true;
    ask_aovs(ask, aovs, follow);
    return ask;
}

// nart_hip_render_halves.  halves_ms: the split and the two half splats.
int render_halves(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* follow, uint32_t aovs, nart_pixel* image,
                  nart_pixel* albedo, nart_pixel* normal, nart_pixel* half_a, nart_pixel* half_b, nart_render_stats* stats,
                  double* halves_ms) {
    if (halves_ms) *halves_ms = 0.0;
    TileGrowthGuard guard(ctx);
    if (!image || !half_a || !half_b) return fail(ctx, NART_E_INVALID, "the half buffers need the beauty's and both halves' image buffers");
    if (const char* why = aov_request_error(aovs, albedo, normal, follow != nullptr)) return fail(ctx, NART_E_INVALID, why);
    const FramePlan plan = plan_frame(halves_ask(p, aovs, follow), PlanRules::Frame);
    FrameRequest rq;
    aovs_to_host(rq, plan, follow != nullptr, image, albedo, normal, nullptr);
    rq.to_host(plan, OutputKind::HalfA, half_a);
    rq.to_host(plan, OutputKind::HalfB, half_b);
    PassTimes times;
    const int rc = render_frame(ctx, p, plan, rq, stats, &times);
    if (halves_ms) *halves_ms = times.ms[PASS_HALVES];
    return rc;
}

// ---------------------------------------------------------------- the denoisers' driver (host/denoise_passes.h)
// f(std::integral_constant<int, N>) for the N of Ns that equals n: a planned halo or chunk size into
// the template argument of the kernel to launch.
template <int... Ns, typename F>
void with_constant(int n, F&& f) {
    (void)((n == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...);
}

// The fields the three denoisers' arguments share, from the layout and dp; the tile kernels' grid (one
// lane per cropped pixel) and the finalize kernels' (one lane per pixel of the total image).
void fill_filter(DnFilterArgs& a, const ImageLayout& layout, const nart_denoise_params& dp) {
    layout.fill(a);
    a.step = 1;
    a.normal_squarings = dp.normal_squarings;
    a.sigma_color = dp.sigma_color;
    a.sigma_depth = dp.sigma_depth;
    a.depth_eps = dp.depth_eps;
    a.sigma_coverage = dp.sigma_coverage;
    a.albedo_floor = dp.albedo_floor;
}
dim3 tile_grid(const DnFilterArgs& a) { return dim3((a.W + DN_TW - 1) / DN_TW, (a.H + DN_TH - 1) / DN_TH); }
dim3 total_grid(const DnFilterArgs& a) { return dim3((uint32_t)(((size_t)a.totalW * a.totalH + 255) / 256)); }

// The planes of a work buffer laid out by `w` over npx pixels, once reserve_work has sized it.
struct WorkPlanes {
    DnWorkLayout w;
    size_t npx;
    uint8_t* base = nullptr;
    float4* f4(uint32_t plane) const { return reinterpret_cast<float4*>(base + w.off4(plane, npx)); }
    float* f1(uint32_t plane) const { return reinterpret_cast<float*>(base + w.off1(plane, npx)); }
    float4* guide() const { return f4(w.guide()); }
    float4* centre() const { return f4(w.centre()); }
    // pingpong -1: none
    float4* sig(int pingpong, uint32_t c) const { return pingpong < 0 ? nullptr : f4(w.sig((uint32_t)pingpong, c)); }
    float* cov() const { return f1(w.cov()); }
    float* slope() const { return f1(w.slope()); }
    float* alpha(uint32_t k) const { return f1(w.alpha(k)); }
};
int reserve_work(nart_ctx* ctx, Buf& buf, WorkPlanes& planes, const char* what) {
    if (int rc = reserve(ctx, buf, ctx->device, planes.npx * planes.w.bytes_per_pixel(), what)) return rc;
    planes.base = buf.as<uint8_t>();
    return NART_OK;
}

// Walks a planned sequence on `st`: an event before the first launch and one after each, launch(entry)
// puts the entry's kernel on the stream; one synchronisation; then t.ms zeroed and every interval added
// into its entry's slot.  ms: their total, the device time of the run.
template <typename Launch>
int run_denoise_passes(nart_ctx* ctx, DenoiseTimes& t, const DnSequence& seq, hipStream_t st, double* ms, Launch&& launch) {
    HIPCHK(record(t.ev[0], st));
    for (uint32_t k = 0; k < seq.n; ++k) {
        launch(seq.launch[k]);
        HIPCHK(hipGetLastError());
        HIPCHK(record(t.ev[k + 1], st));
    }
    HIPCHK(hipEventSynchronize(t.ev[seq.n].handle()));
    for (double& m : t.ms) m = 0.0;
    double total = 0.0;
    for (uint32_t k = 0; k < seq.n; ++k) {
        float d = 0.f;
        HIPCHK(hipEventElapsedTime(&d, t.ev[k].handle(), t.ev[k + 1].handle()));
        t.ms[seq.launch[k].slot] += d;
        total += d;
    }
    if (ms) *ms = total;
    return NART_OK;
}

// What the nart_hip_denoise*_timings getters share; any pointer may be null.
void denoise_times(const DenoiseTimes& t, double* prepare_ms, double* variance_ms, double* pass_ms, double* finalize_ms) {
    if (prepare_ms) *prepare_ms = t.ms[DN_SLOT_PREPARE];
    if (variance_ms) *variance_ms = t.ms[DN_SLOT_VARIANCE];
    if (pass_ms)
        for (uint32_t k = 0; k < DN_MAX_ITERATIONS; ++k) pass_ms[k] = t.ms[DN_SLOT_PASS0 + k];
    if (finalize_ms) *finalize_ms = t.ms[DN_SLOT_FINALIZE];
}

// ---------------------------------------------------------------- denoiser (device/denoise.h)
// Denoise images of the view: the sequence of plan_denoise_passes (prepare, variance, the a-trous
// passes, finalise); synchronous.  ms: device time.  moment >= 0: the sample-variance mode --
// k_dn_prepare<true> takes the variance from the second-moment image and there is no variance launch
// (its time reads 0).  The work buffer is the context's.
int denoise_device(const Images& v, const nart_denoise_params& dp, int beauty, int albedo, int normal, int moment, int out,
                   hipStream_t st, double* ms) {
    nart_ctx* ctx = v.ctx;
    WorkPlanes w = {DN_WORK_PLAIN, (size_t)v.layout.W * v.layout.H};
    if (int rc = reserve_work(ctx, ctx->d_dn, w, "denoiser work buffers")) return rc;
    const bool sample_variance = moment >= 0;
    DnArgs a;
    fill_filter(a, v.layout, dp);
    a.beauty = v.at(beauty);
    a.albedo = v.at(albedo);
    a.normal = v.at(normal);
    a.moment = sample_variance ? v.at(moment) : nullptr;
    a.out = v.at(out);
    a.guide = w.guide();
    a.centre = w.centre();
    a.cov = w.cov();
    a.slope = w.slope();
    const dim3 grid = tile_grid(a), block(256);
    const DnSequence seq = plan_denoise_passes(dp.iterations, !sample_variance);
    return run_denoise_passes(ctx, ctx->dn, seq, st, ms, [&](const DnLaunch& l) {
        a.sig_in[0] = w.sig(l.in, 0);
        a.sig_out[0] = w.sig(l.out, 0);
        a.step = l.step;
        switch (l.kind) {
            case DnKind::Prepare:
                if (sample_variance) hipLaunchKernelGGL(k_dn_prepare<true>, grid, block, 0, st, a);
                else hipLaunchKernelGGL(k_dn_prepare<false>, grid, block, 0, st, a);
                break;
            case DnKind::Variance: hipLaunchKernelGGL(k_dn_variance, grid, block, 0, st, a); break;
            case DnKind::Atrous:
                with_constant<2, 4, 0>(l.halo, [&](auto R) {
                    hipLaunchKernelGGL(k_dn_atrous<decltype(R)::value>, grid, block, 0, st, a);
                });
                break;
            default: hipLaunchKernelGGL(k_dn_finalize, total_grid(a), block, 0, st, a); break;
        }
    });
}

// dp (null: the defaults) into d for a call that denoises, with the second-moment image or not.
int check_denoise(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, bool sample_variance,
                  nart_denoise_params& d) {
    const char* why = denoise_params_error(dp, d);
    if (!why && sample_variance) why = check_sample_variance(p);
    return why ? fail(ctx, NART_E_INVALID, why) : NART_OK;
}

// nart_hip_denoise (moment null) and nart_hip_denoise_moment.  The images are the context's: 4 (beauty,
// albedo, normal, denoised), or 5 in the sample-variance mode (beauty, albedo, normal, moment, denoised).
int denoise_host(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, const nart_pixel* beauty,
                 const nart_pixel* albedo, const nart_pixel* normal, const nart_pixel* moment, nart_pixel* out,
                 double* denoise_ms) {
    nart_denoise_params d;
    if (int rc = check_denoise(ctx, p, dp, moment != nullptr, d)) return rc;
    if (!ctx->subs.empty())
        return forwarded(ctx, denoise_host(first_device(ctx), p, &d, beauty, albedo, normal, moment, out, denoise_ms));
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    const int n_in = moment ? 4 : 3;
    return host_stage(ctx, p, ctx->d_dn_img, "denoiser images",
                      {{beauty, 1}, {albedo, 1}, {normal, 1}, {moment, moment ? 1u : 0u}}, out, 1, [&](const Images& v) {
                          return denoise_device(v, d, 0, 1, 2, moment ? 3 : -1, n_in, 0, denoise_ms);
                      });
}

// nart_hip_render_denoised and, with sample_variance, nart_hip_render_denoised_moment; with follow,
// nart_hip_render_denoised_guides: the followed guides in the first-hit AOVs' place.
int render_denoised(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, bool sample_variance,
                    nart_pixel* image, nart_pixel* out, nart_render_stats* stats, double* denoise_ms,
                    const nart_guide_params* follow = nullptr) {
    nart_denoise_params d;
    if (int rc = check_denoise(ctx, p, dp, sample_variance, d)) return rc;
    // beauty, both AOVs (and the moment image) into the first of the denoising context's device images,
    // the denoised image after them: nothing passes the host
    FrameAsk ask(p->integrator);
    ask_aovs(ask, NART_AOV_ALBEDO | NART_AOV_NORMAL, follow);
    ask.moment = sample_variance;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    const int n = sample_variance ? 5 : 4;
    return frame_stage(ctx, p, plan, first_device(ctx)->d_dn_img, (uint32_t)n, stats, nullptr, [&](const Images& v) {
        const int b = plan.find(OutputKind::Beauty);
        int rc = denoise_device(v, d, b, plan.find(follow ? OutputKind::GuideAlbedo : OutputKind::Albedo),
                                plan.find(follow ? OutputKind::GuideNormal : OutputKind::Normal),
                                sample_variance ? plan.find(OutputKind::Moment) : -1, n - 1, 0, denoise_ms);
        if (!rc && image) rc = v.download(b, image);
        if (!rc) rc = v.download(n - 1, out);
        return rc;
    });
}

// ---------------------------------------------------------------- cross-filtered denoiser (device/denoise_cross.h)
// Cross-denoise images of the view: the sequence of plan_denoise_passes over both halves; synchronous.
// error < 0: no error image.  The work buffers are temporaries of the call.  ms: device time.
int denoise_cross_device(const Images& v, const nart_denoise_params& dp, int half_a, int half_b, int beauty, int albedo,
                         int normal, int out, int error, hipStream_t st, double* ms) {
    nart_ctx* ctx = v.ctx;
    Buf work;  // freed on return
    WorkPlanes w = {DN_WORK_CROSS, (size_t)v.layout.W * v.layout.H};
    if (int rc = reserve_work(ctx, work, w, "cross denoiser work buffers")) return rc;
    DnxArgs a;
    fill_filter(a, v.layout, dp);
    a.half[0] = v.at(half_a);
    a.half[1] = v.at(half_b);
    a.beauty = v.at(beauty);
    a.albedo = v.at(albedo);
    a.normal = v.at(normal);
    a.out = v.at(out);
    a.error = error >= 0 ? v.at(error) : nullptr;
    a.guide = w.guide();
    a.centre = w.centre();
    a.cov = w.cov();
    a.slope = w.slope();
    const dim3 grid = tile_grid(a), block(256);
    return run_denoise_passes(ctx, ctx->dnx, plan_denoise_passes(dp.iterations, true), st, ms, [&](const DnLaunch& l) {
        for (uint32_t h = 0; h < 2; ++h) {
            a.sig_in[h] = w.sig(l.in, h);
            a.sig_out[h] = w.sig(l.out, h);
        }
        a.step = l.step;
        switch (l.kind) {
            case DnKind::Prepare: hipLaunchKernelGGL(k_dnx_prepare, grid, block, 0, st, a); break;
            case DnKind::Variance: hipLaunchKernelGGL(k_dnx_variance, grid, block, 0, st, a); break;
            case DnKind::Atrous:
                with_constant<2, 4, 0>(l.halo, [&](auto R) {
                    hipLaunchKernelGGL(k_dnx_atrous<decltype(R)::value>, grid, block, 0, st, a);
                });
                break;
            default: hipLaunchKernelGGL(k_dnx_finalize, total_grid(a), block, 0, st, a); break;
        }
    });
}

// dp (null: the defaults) into d for a call that cross-denoises: two halves need two samples.
int check_denoise_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, nart_denoise_params& d) {
    const char* why = denoise_params_error(dp, d);
    if (!why && p->spp < 2) why = "cross-filtered denoising needs spp >= 2: a half buffer of its own for each half";
    return why ? fail(ctx, NART_E_INVALID, why) : NART_OK;
}

// nart_hip_denoise_cross.  The images are temporaries of the call: the five inputs, the denoised image and
// the error image.
int denoise_cross_host(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, const nart_pixel* half_a,
                       const nart_pixel* half_b, const nart_pixel* beauty, const nart_pixel* albedo, const nart_pixel* normal,
                       nart_pixel* out, nart_pixel* error, double* denoise_ms) {
    nart_denoise_params d;
    if (int rc = check_denoise_cross(ctx, p, dp, d)) return rc;
    if (!ctx->subs.empty())
        return forwarded(ctx, denoise_cross_host(first_device(ctx), p, &d, half_a, half_b, beauty, albedo, normal, out, error,
                                                 denoise_ms));
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    Buf imgs;  // freed on return
    Images v(ctx, p);
    if (int rc = v.in(imgs, 7, "cross denoiser images")) return rc;
    const nart_pixel* in[5] = {half_a, half_b, beauty, albedo, normal};
    for (size_t i = 0; i < 5; ++i)
        if (int rc = v.upload(i, in[i])) return rc;
    if (int rc = denoise_cross_device(v, d, 0, 1, 2, 3, 4, 5, error ? 6 : -1, 0, denoise_ms)) return rc;
    if (int rc = v.download(5, out)) return rc;
    return error ? v.download(6, error) : NART_OK;
}

// nart_hip_render_denoised_cross: the beauty, the AOVs or followed guides and the two halves into device
// images of the first device, the denoised and the error image after them: nothing passes the host.
int render_denoised_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                          const nart_guide_params* follow, nart_pixel* out, nart_pixel* error, nart_pixel* image,
                          nart_render_stats* stats, double* denoise_ms) {
    nart_denoise_params d;
    if (int rc = check_denoise_cross(ctx, p, dp, d)) return rc;
    const FramePlan plan = plan_frame(halves_ask(p, NART_AOV_ALBEDO | NART_AOV_NORMAL, follow), PlanRules::Frame);
    TileGrowthGuard guard(ctx);
    Buf imgs;  // freed on return
    const uint32_t n = 7;
    return frame_stage(ctx, p, plan, imgs, n, stats, nullptr, [&](const Images& v) {
        const int b = plan.find(OutputKind::Beauty);
        int rc = denoise_cross_device(v, d, plan.find(OutputKind::HalfA), plan.find(OutputKind::HalfB), b,
                                      plan.find(follow ? OutputKind::GuideAlbedo : OutputKind::Albedo),
                                      plan.find(follow ? OutputKind::GuideNormal : OutputKind::Normal), 5, 6, 0, denoise_ms);
        if (!rc && image) rc = v.download(b, image);
        if (!rc) rc = v.download(5, out);
        if (!rc) rc = v.download(6, error);
        return rc;
    });
}

// ---------------------------------------------------------------- firefly cascade (device/cascade.h)
// The reweighting over images of the view: the beauty, the K layer images back to back, the robust
// image out; synchronous.  The time goes to the view's context (cas_ms[1]).
int cascade_device(const Images& v, const nart_cascade_params& cp, const CascadeLevels& lv, uint32_t spp, int beauty,
                   int layers, int out, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    CascadeReweightArgs a;
    a.beauty = v.at(beauty);
    a.layers = v.at(layers);
    a.out = v.at(out);
    v.layout.fill(a);
    a.K = lv.K;
    a.N = (float)spp;
    a.kappa = cp.kappa;
    for (uint32_t j = 0; j < CASCADE_MAX_LAYERS; ++j) a.b[j] = j < lv.K ? lv.b[j] : 0.f;
    return timed(ctx, ctx->ev_cas, st, &ctx->cas_ms[1], [&]() -> int {
        // the border stays zero: the kernel writes the cropped pixels only
        if (int rc = v.zero_async(out, 1, st)) return rc;
        const dim3 grid((a.W + CS_TW - 1) / CS_TW, (a.H + CS_TH - 1) / CS_TH), block(CS_TW * CS_TH);
        hipLaunchKernelGGL(k_cascade_reweight, grid, block, (size_t)lv.K * CS_PLANE * sizeof(float), st, a);
        HIPCHK(hipGetLastError());
        return NART_OK;
    });
}

// nart_hip_render_cascade: the beauty and the K layers, the robust image after them.
int render_cascade(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params& cp, const CascadeLevels& lv,
                   nart_pixel* image, nart_pixel* beauty, nart_pixel* layers, nart_render_stats* stats) {
    ctx->cas_ms[0] = first_device(ctx)->cas_ms[1] = 0.0;  // (the reweighting's time is kept where it runs)
    TileGrowthGuard guard(ctx);
    Buf imgs;  // the device images of the call, on device 0; freed on return
    const uint32_t K = lv.K;
    FrameAsk ask(p->integrator);
    ask.cascade = lv;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    PassTimes times;
    const int rc = frame_stage(ctx, p, plan, imgs, K + 2, stats, &times, [&](const Images& v) {
        // the plan's images back to back (the layers follow one another), the robust image after them
        const int b = plan.find(OutputKind::Beauty), l = plan.find(OutputKind::Layer, 0), o = (int)plan.n_outputs;
        int rc = cascade_device(v, cp, lv, p->spp, b, l, o, 0);
        if (!rc) rc = v.download(o, image);
        if (!rc && beauty) rc = v.download(b, beauty);
        if (!rc && layers) rc = v.download(l, layers, K);
        return rc;
    });
    ctx->cas_ms[0] = times.ms[PASS_CASCADE];
    return rc;
}

// nart_hip_cascade_reweight.
int cascade_host(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params& cp, const CascadeLevels& lv,
                 const nart_pixel* beauty, const nart_pixel* layers, nart_pixel* image) {
    ctx->cas_ms[0] = first_device(ctx)->cas_ms[1] = 0.0;  // (the reweighting's time is kept where it runs)
    if (!ctx->subs.empty()) return forwarded(ctx, cascade_host(first_device(ctx), p, cp, lv, beauty, layers, image));
    const uint32_t K = lv.K;
    Buf imgs;  // the beauty, the layers, the robust image; freed on return
    return host_stage(ctx, p, imgs, "cascade images", {{beauty, 1}, {layers, K}}, image, 1,
                      [&](const Images& v) { return cascade_device(v, cp, lv, p->spp, 0, 1, (int)K + 1, 0); });
}

// ---------------------------------------------------------------- first-hit ID mattes (device/matte.h)
// The ranking over images of the view: the planes back to back (none with no ids), the R / 2 rank
// images out; synchronous.  The time goes to the view's context (mat_ms[1]).
int matte_rank_device(const Images& v, uint32_t n_ids, uint32_t R, int planes, int ranks, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    MatteRankArgs a;
    a.planes = n_ids ? v.at(planes) : nullptr;
    a.out = v.at(ranks);
    v.layout.fill(a);
    a.n_ids = n_ids;
    a.R = R;
    return timed(ctx, ctx->ev_mat, st, &ctx->mat_ms[1], [&]() -> int {
        // the border stays zero: the kernel writes the cropped pixels only
        if (int rc = v.zero_async(ranks, R / 2, st)) return rc;
        const dim3 grid((a.W + MT_TW - 1) / MT_TW, (a.H + MT_TH - 1) / MT_TH), block(MT_LANES);
        const size_t lds = (size_t)((n_ids + 3) / 4) * 4 * MT_LANES * sizeof(float);
        hipLaunchKernelGGL(k_matte_rank, grid, block, lds, st, a);
        HIPCHK(hipGetLastError());
        return NART_OK;
    });
}

// The matte of the ids in `mask` from the R / 2 rank images of the view.
int matte_extract_device(const Images& v, uint32_t R, uint64_t mask, int ranks, int out, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    if (int rc = v.zero_async(out, 1, st)) return rc;  // the border stays zero
    MatteExtractArgs a;
    a.ranks = v.at(ranks);
    a.out = v.at(out);
    v.layout.fill(a);
    a.R = R;
    a.mask = mask;
    const uint64_t n = (uint64_t)a.W * a.H;
    hipLaunchKernelGGL(k_matte_extract, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(hipGetLastError());
    return NART_OK;
}

// nart_hip_render_mattes: the planes (and the beauty, if asked for), the rank images after them.  A
// scene without ids renders no plane: its ranks are empty.
int render_mattes(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params& mp, nart_pixel* ranks,
                  nart_pixel* image, nart_pixel* planes, nart_render_stats* stats) {
    nart_ctx* c0 = first_device(ctx);
    ctx->mat_ms[0] = c0->mat_ms[1] = 0.0;  // (the ranking's time is kept where it runs)
    FrameAsk ask(p->integrator);
    ask.beauty = image != nullptr;
    ask.matte.on = true;
    ask.matte.kind = mp.kind;
    ask.matte.n_ids = mp.kind == NART_MATTE_MATERIAL ? c0->num_materials : c0->num_meshes;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is allocated)
    TileGrowthGuard guard(ctx);
    Buf imgs;  // the device images of the call, on device 0; freed on return
    const uint32_t n_ids = ask.matte.n_ids, P = ask.matte.planes(), R = mp.ranks;
    PassTimes times;
    const int rc = frame_stage(ctx, p, plan, imgs, plan.n_outputs + R / 2, stats, &times, [&](const Images& v) {
        // the plan's images back to back (the planes follow one another), the rank images after them
        const int pl = P ? plan.find(OutputKind::Plane, 0) : 0, rk = (int)plan.n_outputs;
        int rc = matte_rank_device(v, n_ids, R, pl, rk, 0);
        if (!rc) rc = v.download(rk, ranks, R / 2);
        if (!rc && image) rc = v.download(plan.find(OutputKind::Beauty), image);
        if (!rc && planes) rc = v.download(pl, planes, P);
        return rc;
    });
    ctx->mat_ms[0] = times.ms[PASS_MATTE];
    return rc;
}

// nart_hip_matte_rank.
int matte_rank_host(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params& mp, uint32_t n_ids,
                    const nart_pixel* planes, nart_pixel* ranks) {
    ctx->mat_ms[0] = first_device(ctx)->mat_ms[1] = 0.0;
    if (!ctx->subs.empty()) return forwarded(ctx, matte_rank_host(first_device(ctx), p, mp, n_ids, planes, ranks));
    const uint32_t P = (n_ids + 3) / 4, R = mp.ranks;
    Buf imgs;  // the planes, the rank images; freed on return
    return host_stage(ctx, p, imgs, "matte images", {{planes, P}}, ranks, R / 2,
                      [&](const Images& v) { return matte_rank_device(v, n_ids, R, 0, (int)P, 0); });
}

// nart_hip_matte_extract.
int matte_extract_host(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params& mp, const nart_pixel* ranks,
                       uint64_t id_mask, nart_pixel* out) {
    if (!ctx->subs.empty()) return forwarded(ctx, matte_extract_host(first_device(ctx), p, mp, ranks, id_mask, out));
    const uint32_t R = mp.ranks;
    Buf imgs;  // the rank images, the matte; freed on return
    return host_stage(ctx, p, imgs, "matte images", {{ranks, R / 2}}, out, 1,
                      [&](const Images& v) { return matte_extract_device(v, R, id_mask, 0, (int)R / 2, 0); });
}

// ---------------------------------------------------------------- light groups (device/lightgroup.h)
// The mix over images of the view: the G group images back to back, the mixed image out; synchronous.
// gains: [G][3].  The time goes to the view's context (lg_ms[1]).
int light_mix_device(const Images& v, uint32_t G, const float* gains, int groups, int out, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    LightMixArgs a;
    a.groups = v.at(groups);
    a.out = v.at(out);
    v.layout.fill(a);
    a.G = G;
    for (uint32_t g = 0; g < LIGHT_GROUPS_MAX; ++g)
        for (uint32_t c = 0; c < 3; ++c) a.gains[g][c] = g < G ? gains[3 * g + c] : 0.f;
    return timed(ctx, ctx->ev_mix, st, &ctx->lg_ms[1], [&]() -> int {
        const uint64_t n = (uint64_t)a.totalW * a.totalH;  // every pixel, the border too
        hipLaunchKernelGGL(k_light_mix, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        return NART_OK;
    });
}

// nart_hip_light_mix.
int light_mix_host(nart_ctx* ctx, const nart_render_params* p, uint32_t G, const float* gains, const nart_pixel* groups,
                   nart_pixel* out) {
    first_device(ctx)->lg_ms[1] = 0.0;  // (the mix's time is kept where it runs)
    if (!ctx->subs.empty()) return forwarded(ctx, light_mix_host(first_device(ctx), p, G, gains, groups, out));
    Buf imgs;  // the group images, the mixed image; freed on return
    return host_stage(ctx, p, imgs, "light-group images", {{groups, G}}, out, 1,
                      [&](const Images& v) { return light_mix_device(v, G, gains, 0, (int)G, 0); });
}

// nart_hip_render_light_groups: the beauty and the G group images.  map: the group of every light,
// validated by the caller.
int render_light_groups(nart_ctx* ctx, const nart_render_params* p, const uint32_t* map, uint32_t G, nart_pixel* groups,
                        nart_pixel* image, nart_render_stats* stats) {
    ctx->lg_ms[0] = 0.0;
    FrameAsk ask(p->integrator);
    ask.light_groups = G;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is allocated)
    if (int rc = set_light_groups(ctx, map)) return rc;
    TileGrowthGuard guard(ctx);
    FrameRequest rq;
    rq.to_host(plan, OutputKind::Beauty, image);
    for (uint32_t g = 0; g < G; ++g) rq.dst[plan.find(OutputKind::LightGroup, g)] = groups + g * ImageLayout(p).img_floats / 5;
    const int rc = render_frame(ctx, p, plan, rq, stats);
    for (const nart_ctx* c : ctx->subs) ctx->lg_ms[0] = std::max(ctx->lg_ms[0], c->lg_ms[0]);  // the slowest device's
    return rc;
}

// ---------------------------------------------------------------- depth cuts (device/depthcut.h)
// The layers over images of the view: the K cut images back to back, the beauty, the K + 1 layers out;
// synchronous.  The time goes to the view's context (dc_ms[1]).
int depth_layers_device(const Images& v, uint32_t K, int cuts, int beauty, int out, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    DepthLayersArgs a;
    a.cuts = v.at(cuts);
    a.beauty = v.at(beauty);
    a.out = v.at(out);
    v.layout.fill(a);
    a.K = K;
    return timed(ctx, ctx->ev_layers, st, &ctx->dc_ms[1], [&]() -> int {
        const uint64_t n = (uint64_t)a.totalW * a.totalH;  // every pixel, the border too
        hipLaunchKernelGGL(k_depth_layers, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        return NART_OK;
    });
}

// nart_hip_depth_layers.
int depth_layers_host(nart_ctx* ctx, const nart_render_params* p, uint32_t K, const nart_pixel* cuts, const nart_pixel* beauty,
                      nart_pixel* out) {
    first_device(ctx)->dc_ms[1] = 0.0;  // (the layers' time is kept where they run)
    if (!ctx->subs.empty()) return forwarded(ctx, depth_layers_host(first_device(ctx), p, K, cuts, beauty, out));
    Buf imgs;  // the cut images, the beauty, the layers; freed on return
    return host_stage(ctx, p, imgs, "depth-cut images", {{cuts, K}, {beauty, 1}}, out, K + 1,
                      [&](const Images& v) { return depth_layers_device(v, K, 0, (int)K, (int)K + 1, 0); });
}

// nart_hip_render_depth_cuts: the beauty and the K cut images.  cuts: validated by the caller.
int render_depth_cuts(nart_ctx* ctx, const nart_render_params* p, const uint32_t* cuts, uint32_t K, nart_pixel* cut_images,
                      nart_pixel* image, nart_render_stats* stats) {
    ctx->dc_ms[0] = 0.0;
    FrameAsk ask(p->integrator);
    ask.depth_cuts = K;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is allocated)
    set_depth_cuts(ctx, cuts, K);
    TileGrowthGuard guard(ctx);
    FrameRequest rq;
    rq.to_host(plan, OutputKind::Beauty, image);
    for (uint32_t j = 0; j < K; ++j) rq.dst[plan.find(OutputKind::DepthCut, j)] = cut_images + j * ImageLayout(p).img_floats / 5;
    const int rc = render_frame(ctx, p, plan, rq, stats);
    for (const nart_ctx* c : ctx->subs) ctx->dc_ms[0] = std::max(ctx->dc_ms[0], c->dc_ms[0]);  // the slowest device's
    return rc;
}

// ---------------------------------------------------------------- denoised parts (device/denoise_parts.h)
// Denoise K part images of the layout with shared guides, on ctx's device (current): the sequence of
// plan_denoise_parts_passes -- prepare once, the rest per chunk of the plan (host/denoise_parts_plan.h;
// NART_DN_PARTS_CHUNK forces the chunks' size), and with `sum` the sum of the outputs; synchronous.  sum
// may be one of the part images (they are consumed by prepare), not an output.  The work buffers are
// temporaries of the call.  ms: device time.
int denoise_parts_device(nart_ctx* ctx, const ImageLayout& layout, const nart_denoise_params& dp, uint32_t K,
                         const float* const* parts, const float* albedo, const float* normal, float* const* out, float* sum,
                         hipStream_t st, double* ms) {
    const char* knob = env_opt("NART_DN_PARTS_CHUNK");
    const PartsPlan plan = plan_denoise_parts(K, knob && *knob ? (uint32_t)std::max(0, std::atoi(knob)) : 0u);
    Buf work;  // freed on return
    WorkPlanes w = {dn_work_parts(K), (size_t)layout.W * layout.H};
    if (int rc = reserve_work(ctx, work, w, "denoised parts work buffers")) return rc;
    DnpArgs a = {};
    fill_filter(a, layout, dp);
    a.albedo = albedo;
    a.normal = normal;
    a.guide = w.guide();
    a.ad = w.centre();
    a.cov = w.cov();
    a.slope = w.slope();
    const dim3 grid = tile_grid(a), block(256);
    const DnSequence seq = plan_denoise_parts_passes(plan, dp.iterations, sum != nullptr);
    return run_denoise_passes(ctx, ctx->dnp, seq, st, ms, [&](const DnLaunch& l) {
        if (l.kind == DnKind::Sum) {
            PartsSumArgs s = {};
            for (uint32_t k = 0; k < K; ++k) s.in[k] = out[k];
            s.out = sum;
            s.n = K;
            s.n_pixels = (uint64_t)a.totalW * a.totalH;
            hipLaunchKernelGGL(k_parts_sum, total_grid(a), block, 0, st, s);
            return;
        }
        // prepare takes all K parts, the others the parts of their chunk in the slots 0 .. n - 1
        const bool prepare = l.kind == DnKind::Prepare;
        const uint32_t first = prepare ? 0 : plan.first[l.chunk];
        a.n = prepare ? K : plan.size[l.chunk];
        for (uint32_t c = 0; c < a.n; ++c) {
            a.part[c] = prepare ? parts[c] : nullptr;
            a.sig_in[c] = w.sig(l.in, first + c);
            a.sig_out[c] = w.sig(l.out, first + c);
            a.alpha[c] = w.alpha(first + c);
            a.out[c] = out[first + c];
        }
        a.step = l.step;
        switch (l.kind) {
            case DnKind::Prepare: hipLaunchKernelGGL(k_dnp_prepare, grid, block, 0, st, a); break;
            case DnKind::Variance:
                with_constant<1, 2, 3, 4>(a.n, [&](auto C) {
                    hipLaunchKernelGGL(k_dnp_variance<decltype(C)::value>, grid, block, 0, st, a);
                });
                break;
            case DnKind::Atrous:
                with_constant<2, 4, 0>(l.halo, [&](auto R) {
                    with_constant<1, 2, 3, 4>(a.n, [&](auto C) {
                        hipLaunchKernelGGL((k_dnp_atrous<decltype(R)::value, decltype(C)::value>), grid, block, 0, st, a);
                    });
                });
                break;
            default: hipLaunchKernelGGL(k_dnp_finalize, total_grid(a), block, 0, st, a); break;
        }
    });
}

// nart_hip_denoise_parts: the K parts, the albedo, the normal, the K denoised images after them; the sum
// takes the place of part 0, which prepare has consumed by then.  d: validated by the caller.
int denoise_parts_host(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params& d, uint32_t K,
                       const nart_pixel* parts, const nart_pixel* albedo, const nart_pixel* normal, nart_pixel* out,
                       nart_pixel* sum, double* denoise_ms) {
    if (!ctx->subs.empty())
        return forwarded(ctx, denoise_parts_host(first_device(ctx), p, d, K, parts, albedo, normal, out, sum, denoise_ms));
    if (const char* why = check_image_size(p)) return fail(ctx, NART_E_INVALID, why);
    Buf imgs;  // freed on return
    return host_stage(ctx, p, imgs, "denoised parts images", {{parts, K}, {albedo, 1}, {normal, 1}}, out, K,
                      [&](const Images& v) {
                          const float* in[DNP_MAX_PARTS] = {};
                          float* o[DNP_MAX_PARTS] = {};
                          for (uint32_t k = 0; k < K; ++k) in[k] = v.at(k), o[k] = v.at(K + 2 + k);
                          int rc = denoise_parts_device(v.ctx, v.layout, d, K, in, v.at(K), v.at(K + 1), o, sum ? v.at(0) : nullptr,
                                                        0, denoise_ms);
                          if (!rc && sum) rc = v.download(0, sum);
                          return rc;
                      });
}

// nart_hip_render_denoised_light_groups (n_cuts 0: `plan` a light-group frame of K groups) and
// nart_hip_render_denoised_depth_layers (`plan` a depth-cut frame of n_cuts cuts, K = n_cuts + 1 layers):
// two frames back to back into device images of the first device -- the parts' frame, then the guides'
// frame (no beauty: camera rays only; follow: the followed guides in the first-hit AOVs' place) -- then
// the layers, the parts denoise and what the caller asked for to the host.  All images are temporaries
// of the call.  The group map or the cuts are set, and everything validated, by the caller.  stats: the
// parts' frame and the stage; the guides frame's render_ms goes to ctx->dnp_guides_ms.
int render_denoised_parts(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params& d,
                          const nart_guide_params* follow, const FramePlan& plan, uint32_t n_cuts, uint32_t K,
                          nart_pixel* denoised, nart_pixel* sum, nart_pixel* noisy, nart_pixel* image, nart_render_stats* stats,
                          double* denoise_ms) {
    nart_ctx* c0 = first_device(ctx);
    ctx->dnp_guides_ms = 0.0;
    FrameAsk gask(p->integrator);
    gask.beauty = false;
    ask_aovs(gask, NART_AOV_ALBEDO | NART_AOV_NORMAL, follow);
    const FramePlan gplan = plan_frame(gask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is allocated)
    if (gplan.code) return fail(ctx, gplan.code, gplan.message);
    TileGrowthGuard guard(ctx);
    Buf imgs, gimgs;  // the device images of the call, on device 0; freed on return
    const uint32_t L = plan.n_outputs, O = L + (n_cuts ? K : 0), n_images = O + K + 1;
    if (int rc = render_frame(ctx, p, plan, FrameRequest(&imgs, n_images), stats)) return rc;
    nart_render_stats gstats = {};
    if (int rc = render_frame(ctx, p, gplan, FrameRequest(&gimgs, 2), &gstats)) return rc;
    ctx->dnp_guides_ms = gstats.render_ms;
    RenderTimer timer(stats);
    Images v(c0, p), gv(c0, p);
    int rc = v.in(imgs, n_images, "image");  // (sized by the frames: this lays them out)
    if (!rc) rc = gv.in(gimgs, 2, "image");
    const int b = plan.find(OutputKind::Beauty);
    if (!rc && n_cuts) rc = depth_layers_device(v, n_cuts, plan.find(OutputKind::DepthCut, 0), b, (int)L, 0);
    const float* in[DNP_MAX_PARTS] = {};
    float* o[DNP_MAX_PARTS] = {};
    for (uint32_t k = 0; k < K; ++k) {
        in[k] = n_cuts ? v.at(L + k) : v.at(plan.find(OutputKind::LightGroup, k));
        o[k] = v.at(O + k);
    }
    if (!rc)
        rc = denoise_parts_device(c0, v.layout, d, K, in, gv.at(gplan.find(follow ? OutputKind::GuideAlbedo : OutputKind::Albedo)),
                                  gv.at(gplan.find(follow ? OutputKind::GuideNormal : OutputKind::Normal)), o,
                                  sum ? v.at(O + K) : nullptr, 0, denoise_ms);
    if (!rc) rc = v.download(O, denoised, K);
    if (!rc && sum) rc = v.download(O + K, sum);
    for (uint32_t k = 0; k < K && !rc && noisy; ++k)
        rc = v.download(n_cuts ? L + k : plan.find(OutputKind::LightGroup, k), noisy + k * (v.layout.img_floats / 5));
    if (!rc && image) rc = v.download(b, image);
    return forwarded(ctx, rc);
}

// ---------------------------------------------------------------- cost image (device/cost.h)
// The grid of traced pixels of p (include/nart_hip.h, "Cost image"): RenderTile's x, y range.
void cost_grid_of(const nart_render_params* p, uint32_t* w, uint32_t* h) {
    nart_session_geometry g;
    nart_session_geometry_of(p, &g);
    *w = std::min(p->bucket_size * g.n_buckets_x, g.total_width);
    *h = std::min(p->bucket_size * g.n_buckets_y, g.total_height);
}

// A host cost grid into image `out` of the view; synchronous.  The time goes to the view's context
// (cost_ms[1]).
int cost_image_device(const Images& v, const nart_render_params* p, const nart_cost_pixel* cost, int out, hipStream_t st) {
    nart_ctx* ctx = v.ctx;
    CostImageArgs a;
    cost_grid_of(p, &a.grid_w, &a.grid_h);
    const size_t n = (size_t)a.grid_w * a.grid_h;
    Buf grid;  // the grid on the device; freed on return
    if (int rc = reserve(ctx, grid, ctx->device, n * sizeof(uint4), "cost grid")) return rc;
    HIPCHK(hipMemcpy(grid.as<void>(), cost, n * sizeof(uint4), hipMemcpyHostToDevice));
    a.grid = grid.as<uint4>();
    a.out = v.at(out);
    a.spp = p->spp;
    v.layout.fill(a);
    if (int rc = v.zero_async(out, 1, st)) return rc;
    return timed(ctx, ctx->ev_cost_img, st, &ctx->cost_ms[1], [&]() -> int {
        hipLaunchKernelGGL(k_cost_image, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
        HIPCHK(hipGetLastError());
        return NART_OK;
    });
}

// nart_hip_cost_image.
int cost_image_host(nart_ctx* ctx, const nart_render_params* p, const nart_cost_pixel* cost, nart_pixel* image) {
    first_device(ctx)->cost_ms[1] = 0.0;  // (the image's time is kept where it runs)
    if (!ctx->subs.empty()) return forwarded(ctx, cost_image_host(first_device(ctx), p, cost, image));
    Buf imgs;  // the image; freed on return
    return host_stage(ctx, p, imgs, "cost image", {}, image, 1,
                      [&](const Images& v) { return cost_image_device(v, p, cost, 0, 0); });
}

// A cost frame's grid on one device's context: sized for p and zero (every device of a multi-device
// context reduces its own buckets into its own grid).
int cost_grid_begin(nart_ctx* ctx, uint32_t gw, uint32_t gh) {
    HIPCHK(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)gw * gh * sizeof(uint4);
    if (int rc = reserve(ctx, ctx->d_cost_grid, ctx->device, bytes, "cost grid")) return rc;
    HIPCHK(hipMemset(ctx->d_cost_grid.as<void>(), 0, bytes));
    ctx->cost_grid_w = gw;
    ctx->cost_grid_h = gh;
    return NART_OK;
}

// nart_hip_render_cost: the beauty (if asked for) and the cost grid.  The devices' grids are added on
// the host: every pixel is non-zero on exactly one of them.
int render_cost(nart_ctx* ctx, const nart_render_params* p, nart_cost_pixel* cost, nart_pixel* image,
                nart_render_stats* stats) {
    ctx->cost_ms[0] = 0.0;
    FrameAsk ask(p->integrator);
    ask.cost = true;
    const FramePlan plan = plan_frame(ask, PlanRules::Frame);
    if (plan.code) return fail(ctx, plan.code, plan.message);  // (before anything is allocated)
    int rc = forwarded(ctx, check_params(first_device(ctx), p));
    if (rc) return rc;
    uint32_t gw = 0, gh = 0;
    cost_grid_of(p, &gw, &gh);
    std::vector<nart_ctx*> devs = ctx->subs;
    if (devs.empty()) devs.push_back(ctx);
    for (nart_ctx* c : devs)
        if ((rc = cost_grid_begin(c, gw, gh))) return c == ctx ? rc : fail(ctx, rc, c->err);
    TileGrowthGuard guard(ctx);
    FrameRequest rq;
    rq.to_host(plan, OutputKind::Beauty, image);
    if ((rc = render_frame(ctx, p, plan, rq, stats))) return rc;
    const size_t n = (size_t)gw * gh;
    std::vector<nart_cost_pixel> part(devs.size() > 1 ? n : 0);
    for (size_t d = 0; d < devs.size(); ++d) {
        nart_ctx* c = devs[d];
        nart_cost_pixel* dst = d ? part.data() : cost;
        if (hipSetDevice(c->device) != hipSuccess ||
            hipMemcpy(dst, c->d_cost_grid.as<void>(), n * sizeof(uint4), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, NART_E_HIP, "copy cost grid");
        }
        for (size_t i = 0; d && i < n; ++i) {
            cost[i].rays_extend += dst[i].rays_extend;
            cost[i].rays_shadow += dst[i].rays_shadow;
            cost[i].hits += dst[i].hits;
            cost[i].steps += dst[i].steps;
        }
        ctx->cost_ms[0] = std::max(ctx->cost_ms[0], c->cost_ms[0]);  // the slowest device's
    }
    return NART_OK;
}

}  // namespace
