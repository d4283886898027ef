/*
 * nart_hip.h — MI355X (gfx950) render path, C ABI.
 *
 * Replaces the reference's per-session hot path
 *     std::vector<Pixel> RenderSession::Render() const      src/core/render.cpp:114-206
 * (bucket loop + per-pixel RNG seed + Latin square + Camera::CastRay + Integrator::Li_alpha +
 *  AddSample Gaussian splat + bucket-raster tile combine) with HIP kernels on one device.
 * Li_alpha (src/integrators/pathintegrator.cpp:144-259) with its BVH traversal
 * (src/core/bvh.cpp:132-176), BSDFs (src/core/bxdf.cpp, src/bxdfs/<name>.cpp), materials
 * (src/materials/<type>material.cpp) and lights (src/lights/<type>light.cpp) run on the device.
 *
 * All entry points return NART_OK (0) or a negative NART_E_* code (nart_scene.h); no C++
 * exception crosses the ABI and nothing aborts.  A context owns all device memory of its
 * device(s) (and, multi-device, its streams and RCCL communicator) and is not thread-safe (one
 * caller thread, like the reference's main thread).
 */
#ifndef NART_HIP_H
#define NART_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "nart_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nart_ctx nart_ctx;

typedef struct nart_render_stats {
    double render_ms;       /* wall time of the render call (host clock)               */
    double kernel_ms;       /* device time of the path-tracing kernels (HIP events)     */
    double splat_ms;        /* device time of the splat + combine kernels               */
    uint32_t kernel_launches; /* number of path-tracing kernel launches timed in kernel_ms */
    uint32_t schedule;      /* NART_SCHED_* bits: the scheduling paths the render took (OR over
                               its launches; observability for tests and benches)         */
    uint64_t samples;       /* camera samples counted in the metric (W*H*spp share)     */
    uint64_t traced_samples;/* samples actually traced (incl. extra rows, render.cpp:164) */
    /* Counter pass only (nart_hip_set_counters(ctx,1)); zero otherwise.
     * rays_extend, bounces and rays_shadow are path counts: each accepted sample's, whichever lane
     * or schedule ran it (a speculative lane's sample counts once it is verified, a dropped one
     * never), so they depend only on the scene and the session.
     *   rays_extend  closest-hit queries: the camera ray of every traced sample with a bounce limit
     *                above zero, plus one per continued bounce (pathintegrator.cpp:184)
     *   bounces      "shaded" hits: extension queries that found a surface, i.e. every hit the
     *                integrator processes -- a BSDF is built for it; where the nested-dielectric
     *                list admits it, EstimateDirect and the continuation sample follow, otherwise
     *                (a lower-priority interface) the path only steps through it
     *   rays_shadow  occlusion queries of EstimateDirect actually traced: the device skips a query
     *                whose term is exactly zero, so this is at most the reference's two per valid hit
     * node_visits, tri_tests (and octree_checks, octree_replays below) are traversal work, added by
     * whichever lane traces a ray: they include the speculative lanes' dropped samples and the
     * packet traversal of the camera rays, so they do depend on the schedule. */
    uint64_t rays_extend, rays_shadow, node_visits, tri_tests, bounces;
    double latin_ms;        /* device time of the LatinSquare kernel                    */
    /* Counter pass only: hits whose octree reachability needed the exact ancestor-chain check,
     * and queries answered by replaying the reference octree search (device/octree.h). */
    uint64_t octree_checks, octree_replays;
    double primary_ms;      /* part of kernel_ms: the camera-ray kernel that runs before the path
                               kernel (k_primary, default variant only)                  */
} nart_render_stats;

/* nart_render_stats.schedule bits */
#define NART_SCHED_PROBE_QUEUE 0x1u  /* cost probe + pixel queue, persistent refill lanes          */
#define NART_SCHED_PRIORITY    0x2u  /* priority lanes for the costliest pixels (ray-queue kernel) */
#define NART_SCHED_SPEC_PAIRS  0x4u  /* speculative lane groups on the costliest pixels            */
#define NART_SCHED_WAVE_GROUPS 0x8u  /* wave-group refill in probe order (ray-queue kernel)        */
#define NART_SCHED_VOL_QUEUE   0x10u /* volume kernel: cost probe, costliest groups first          */
#define NART_SCHED_VOL_SPARSE  0x20u /* volume kernel: sparse waves for the costliest groups       */
#define NART_SCHED_SPLAT_SKEW  0x40u /* skewed-time splat (k_splat_skew)                           */
#define NART_SCHED_PRIMARY     0x80u /* camera rays traced first (k_primary)                       */
#define NART_SCHED_SPLAT_ROWS  0x100u /* skewed-time splat, W lanes per tile column (k_splat_rows)  */
#define NART_SCHED_HALF_WAVES  0x200u /* costliest pixels on one wave per SIMD, raised priority     */
#define NART_SCHED_SPECIALIZED 0x400u /* a scene-specialised path-kernel build ran (nart_hip_set_specialize) */
#define NART_SCHED_LEAN        0x800u /* the lean three-waves-per-SIMD build of a throughput-bound launch */

/* Upload the scene, build the device BVH.  device_id: HIP ordinal. */
int nart_hip_create(const nart_scene_blob* scene, int device_id, nart_ctx** out);
void nart_hip_destroy(nart_ctx* ctx);
const char* nart_hip_last_error(const nart_ctx* ctx);

/* Multi-GPU context over device_ids[0..n_devices) of this node, replacing the reference's
   tbb::task_group over host cores (render.cpp:152-177): the scene is uploaded to every device;
   nart_hip_render shards the buckets (dealt in a low-discrepancy order, nart_hip_shard_buckets), renders
   the shares concurrently (one host thread per device), gathers the tiles to device_ids[0] with
   the library's own RCCL communicator (ncclCommInitAll over the list; ncclSend/ncclRecv over
   xGMI) and combines them there in bucket raster order (render.cpp:183-203), so the image is
   bit-identical for any n.  n_devices == 1 is exactly nart_hip_create.  Repeated ordinals (a
   rehearsal of n devices on fewer GPUs) gather with device copies, since RCCL needs distinct
   GPUs; NART_GATHER=rccl|copy overrides (read at creation).  If librccl cannot be loaded or
   ncclCommInitAll fails, the context falls back to the device-copy gather (same image;
   nart_hip_context_devices reports it); only NART_GATHER=rccl then fails with NART_E_RCCL.
   A gather that fails inside the RCCL group still closes the group (ncclGroupEnd), returns
   NART_E_RCCL and marks the context unusable: every later render returns NART_E_RCCL, and the
   caller destroys the context and creates a new one. */
int nart_hip_create_multi(const nart_scene_blob* scene, const int* device_ids, int n_devices, nart_ctx** out);

/* Devices of a context (1 for nart_hip_create) and its gather: uses_rccl = 1 RCCL, 0 device
   copies, 2 device copies because RCCL was unavailable (the fallback above). */
int nart_hip_context_devices(const nart_ctx* ctx, int* n_devices, int* uses_rccl);

/* Test hook (no reference counterpart): fault 1 makes the next RCCL gather of a multi-device
   context post a send to a rank that does not exist, exercising the failure path above; 0 clears.
   No effect on device-copy gathers. */
int nart_hip_debug_fault(nart_ctx* ctx, int fault);

/* HIP devices visible to this process. */
int nart_hip_device_count(int* count);

/* Host only: the buckets device device_index of n_devices renders, ascending, into ids (may be
   null to query the count).  A diagonal lattice: bucket id b = by*n_buckets_x + bx goes to device
   (bx + s*by) % n_devices, s the step in [1, n) coprime to n closest to 0.382 n (3 for 8 devices),
   so every region of the frame splits evenly over the devices (nart_amd/dist.py bucket_owners). */
int nart_hip_shard_buckets(uint32_t n_buckets_x, uint32_t n_buckets, uint32_t n_devices, uint32_t device_index,
                           uint32_t* ids, uint32_t* count);

/* Whole-session render into device memory: as nart_hip_render, but the combined image stays on
   the (first) device, in a buffer the context owns (valid until the next render or destroy), and
   *d_image points at it -- no PCIe copy.  Multi-device contexts gather the tiles to device 0 with
   their RCCL send/receive group (or device copies) first.  Synchronous. */
int nart_hip_render_device(nart_ctx* ctx, const nart_render_params* p, const nart_pixel** d_image,
                           nart_render_stats* stats);

/* Whole-session render, Render()-equivalent: fills a caller-owned host buffer of
   totalW*totalH nart_pixel (render.cpp:114-206 contract, render.h:18-21 layout). */
int nart_hip_render(nart_ctx* ctx, const nart_render_params* p, nart_pixel* image,
                    nart_render_stats* stats);

/* First-hit AOVs (no reference counterpart): denoiser guide images of the first surface each
   camera sample sees.  The first hit is the triangle Scene::Intersect returns at bounce 0 -- the
   reference octree's answer, bounded by the nearest analytic light in front of it
   (pathintegrator.cpp:167-184); a sample whose camera ray meets a light first, or nothing, is a
   miss, and nested-dielectric validity (IsectIsValid) is not applied.  Per sample
       albedo record {albedo.rgb, hit}:   the hit material's colour pattern at the hit's st (rho_d for
                                          Lambert and plastic, rho_s for specular and glossy, tau for
                                          glass: the texel the BSDF reads); hit = 1
       normal record {normal.xyz, depth}: the normalised shading normal of the BSDF frame (world
                                          space, normal map applied, not flipped towards the camera)
                                          and the hit's t as Triangle::Intersect computes it (the
                                          distance from the camera: the ray direction is unit length)
   and all zeros for a miss.  Each record stream is splatted and combined exactly as Li_alpha is
   (AddSample, render.cpp:23-70; tile combine :183-203) into a nart_pixel image of totalW*totalH:
   contribution / filter_weight_sum is the filtered AOV.  The normal image is therefore a filtered
   average of unit normals and is NOT renormalised.

   nart_hip_render_aovs: aovs = NART_AOV_* bits, each needing its host buffer (totalW*totalH
   nart_pixel); image = the beauty, bit-identical to nart_hip_render's, or null for an AOV-only
   render (LatinSquare, camera rays and the AOV passes: no path kernel).  aov_ms, if non-null,
   receives the device time of the AOV record and AOV splat kernels.  A render without AOV bits
   launches exactly what nart_hip_render launches.  NART_E_INVALID: null ctx or p, a bit without its
   buffer, an unknown bit, or nothing requested; NART_E_UNSUPPORTED: the volume integrator (no
   surfaces).  Multi-device contexts gather the AOV tiles with the beauty's gather. */
#define NART_AOV_ALBEDO 0x1u   /* contribution = {albedo.rgb, hit}    */
#define NART_AOV_NORMAL 0x2u   /* contribution = {normal.xyz, depth}  */
int nart_hip_render_aovs(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, nart_pixel* image,
                         nart_pixel* albedo, nart_pixel* normal, nart_render_stats* stats, double* aov_ms);

/* Second-moment image (no reference counterpart): how noisy each pixel is, from the renderer's own
   samples.  A nart_pixel image of totalW*totalH.  For every tile pixel it accumulates, over the
   samples AddSample (render.cpp:23-70) adds to that pixel and in AddSample's order (source pixel
   raster, then sample index), with w the filter weight the beauty's splat uses for that (sample,
   pixel) pair and (r, g, b, a) the sample's Li_alpha:
       contribution      = { sum (r*r)*w, sum (g*g)*w, sum (b*b)*w, sum w*w }
       filter_weight_sum =   sum w
   every product and sum one float32 operation in the order written, nothing contracted; tiles are
   combined in bucket raster order as every other image is.  filter_weight_sum therefore has the
   beauty's bits, contribution.rgb / filter_weight_sum is the filtered second moment of the radiance,
   and contribution.a / filter_weight_sum^2 is 1 / the effective sample count of the pixel.  It needs
   no surfaces, so it also works for the volume integrator.

   On the device the pass runs after the beauty's splat has consumed the batch's Li_alpha records:
   k_moment squares their colour channels in place (no extra per-sample memory), and the beauty's
   splat kernel runs once more, built with a flag that makes the fourth accumulator add w*w where
   it otherwise adds a*w -- one more pass over the samples.  A render that does not ask for the
   moment image launches exactly what it launched before.

   nart_hip_render_moment: as nart_hip_render_aovs, with aovs allowed to be 0, plus the moment image
   (required).  The moment image needs the path kernel: image may be null, and the path kernel and
   the beauty's splat still run.  moment_ms, if non-null, receives the device time of k_moment plus
   the moment splat.  The beauty and the AOVs have the bits nart_hip_render / nart_hip_render_aovs
   give.  NART_E_INVALID: as nart_hip_render_aovs, or a null moment; NART_E_UNSUPPORTED: an AOV bit
   with the volume integrator.  Multi-device contexts gather the moment tiles with the beauty's. */
int nart_hip_render_moment(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, nart_pixel* image,
                           nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment, nart_render_stats* stats,
                           double* aov_ms, double* moment_ms);

/* Adaptive sampling (no reference counterpart): a pilot pass at few samples, a noise estimate per
   bucket from the bucket's own samples, and more samples only for the buckets that need them.

   Levels: L_0 = min_spp, L_{i+1} = min(L_i * growth, spp), ending on spp = p->spp, the maximum; the
   single level spp if min_spp >= spp; at most 32 levels (the 32nd is spp).  If every bucket refines
   to the top the extra work is at most 1 / (growth - 1) of a uniform render.

   The loop, per device over the buckets the device owns (a multi-device context shards as ever and
   each device refines its own share; the estimate below needs the bucket's own tiles only):
     1. render the listed buckets at L_i: the beauty, the second-moment tiles and the requested AOVs;
     2. k_bucket_error: one float E per listed bucket (below);
     3. the bucket's tiles REPLACE its tiles of the earlier level.  They are not accumulated: a
        pixel's RNG stream is seeded by its coordinates (render.cpp:78-108), so a second pass replays
        the first pass's numbers and the two would be correlated;
     4. a bucket stops iff E <= threshold (a NaN or infinite E refines), or if L_i is the last level;
     5. the buckets that did not stop, in ascending id order, are the next list; an empty list ends
        the loop;
     6. the tiles are combined in bucket raster order and delivered as every other image is.
   Every bucket's tile is therefore, bit for bit, that bucket's tile of a uniform render at the sample
   count the bucket ended on (a bucket's tile never depends on the buckets rendered with it), and the
   second-moment image carries each pixel's effective sample count (sum w^2 / (sum w)^2), so
   nart_hip_denoise_moment works on an adaptive frame unchanged.

   Bucket error E: the relative standard error of the bucket's mean luminance.  All arithmetic is
   float32 + - * / sqrt and comparisons, one operation each, in the order written (nothing
   contracted, divide and sqrt correctly rounded); max(a, b) means a > b ? a : b.  The own pixels of
   bucket (bx, by) are its tile pixels (fb + dx, fb + dy), dx in [0, nx), nx = min(B, total_width -
   B * bx), dy in [0, ny), ny likewise, fb = filter_bounds, B = bucket_size: the splat centres of the
   pixels the bucket traces, extra rows included.  Per own pixel, T the beauty tile pixel and M the
   moment tile pixel (contribution rgba, filter_weight_sum w):
       if T.w > 0:  c  = T.rgb / T.w
                    k  = M.a / (M.w * M.w)
                    per channel ch: m2 = M.ch / M.w, var = max(0, m2 - c.ch * c.ch), V.ch = var * k
                    sd = (0.2126 * sqrt(V.r) + 0.7152 * sqrt(V.g)) + 0.0722 * sqrt(V.b)
                    l  = max((0.2126 * c.r + 0.7152 * c.g) + 0.0722 * c.b, 0)
       else:        sd = 0, l = 0
   Sums start from 0: per row rs[dy] = sum over dx ascending of sd, rl[dy] likewise of l; then
   S = sum over dy ascending of rs[dy], Ls likewise of rl[dy];
       E = S / (Ls + floor * float(nx * ny))
   floor keeps dark buckets from dividing by nothing; a black bucket has E = 0.  E is a pure function
   of the two tiles: no atomics, any launch shape, any place in the list.

   nart_hip_adaptive_levels (host only, no device): the level list for a maximum spp into levels
   (room for 32; null to query *n).  ap null: the defaults.
   nart_hip_render_adaptive: ap null means the defaults.  aovs, image, albedo, normal and moment as in
   nart_hip_render_moment, except that moment may be null (the moment tiles are rendered regardless)
   and that nothing but the per-bucket outputs need be requested.  bucket_spp (uint32[nBucketsX *
   nBucketsY], bucket-id order) receives the sample count each bucket ended on, bucket_error
   (float[same]) the E of that final level (so E is computed at the last level too); both optional.
   stats add up over the levels: samples is the number of samples taken, replaced ones included.
   adaptive_ms, if non-null, receives the device time of the error and scatter kernels over all
   levels (the slowest device's).  No other entry point changes what it launches.
   NART_E_INVALID: as nart_hip_render_aovs, or min_spp < 2, p->spp < 2 (one sample has no variance),
   growth outside 2..16, a threshold that is NaN or < 0 (+inf is allowed: nothing refines), a floor
   that is not finite and > 0.  NART_E_UNSUPPORTED: an AOV bit with the volume integrator (without
   AOV bits the volume integrator works). */
typedef struct nart_adaptive_params {
    uint32_t min_spp;   /* samples of the pilot pass, >= 2                         default 16   */
    uint32_t growth;    /* factor between levels, 2..16                            default 4    */
    float threshold;    /* a bucket stops when its E <= threshold                  default 0.1  */
    float floor;        /* luminance added per pixel to the denominator of E       default 0.01 */
} nart_adaptive_params;
void nart_hip_adaptive_params_init(nart_adaptive_params* ap);
int nart_hip_adaptive_levels(const nart_adaptive_params* ap, uint32_t spp, uint32_t* levels, uint32_t* n);
int nart_hip_render_adaptive(nart_ctx* ctx, const nart_render_params* p, const nart_adaptive_params* ap, uint32_t aovs,
                             nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment,
                             uint32_t* bucket_spp, float* bucket_error, nart_render_stats* stats, double* adaptive_ms);

/* Firefly cascade (no reference counterpart): a robust image next to the beauty, after Zirr, Hanika
   and Dachsbacher, "Re-weighting Firefly Samples for Improved Finite-Sample Monte Carlo Estimates"
   (2018).  Every sample is split by luminance between two neighbouring brightness layers, each layer
   is splatted and combined like any other image, and a layer's contribution to a pixel is trusted
   only as far as the pixel's 3x3 neighbourhood holds enough samples of about that brightness: a real
   highlight or caustic has many, a firefly has one.  Opt-in: no other entry point changes its bits,
   its launches or the memory it finds.

   All arithmetic is float32 + - * / and comparisons, one operation each, in the order written
   (nothing contracted, divide correctly rounded); tests/cascade_py.py restates it in numpy.
   lum(r, g, b) = (0.2126 * r + 0.7152 * g) + 0.0722 * b.

   Levels: b_0 = start, b_{j+1} = b_j * base, j < K = layers, formed on the host in float32.  A level
   that is not finite, or not above the level before it (a denormal start), is NART_E_INVALID.

   Split, per sample record L = {r, g, b, a}, l = lum(r, g, b):
       if !(l - l == 0) (not finite) or l <= b_0:   layer 0 takes the record whole
       else if l > b_{K-1}:                         layer K-1 takes it whole
       else, j the index with b_j < l <= b_{j+1}:
           w_lo = (b_{j+1} / l - 1) / (base - 1),  w_hi = 1 - w_lo
           layer j   gets {r * w_lo, g * w_lo, b * w_lo, a * w_lo}
           layer j+1 gets {r * w_hi, g * w_hi, b * w_hi, a * w_hi}
   and every other layer's record for the sample is exactly {+0, +0, +0, +0}.  In exact arithmetic the
   layers sum to the sample and sum_j w_j * l / b_j = 1, which is what lets a layer's brightness be
   read as a sample count.  (With levels that are powers of two, the defaults among them, both
   weights lie in [0, 1]; another base can round w_lo an ulp beyond 1 right above a level.)

   Layer images: each layer's record stream goes through the beauty's splat plan and the tile combine
   as if it were Li_alpha (the plain splat kernels, unchanged), so every layer image's
   filter_weight_sum has the beauty's bits.  On the device k_cascade_split writes layer j's records
   into a second per-sample record buffer (16 B per sample, held only while the call runs:
   batches are sized for 44 instead of 28 B per sample in such a call) right after the beauty's
   splat, once per layer per batch, each time followed by the plan's splat into that layer's tiles.

   Reweighting (k_cascade_reweight), over the cropped image_width x image_height image (pixel (x, y) is
   total-image pixel (x + fb, y + fb)), per pixel p; C_j layer j's pixel, W = beauty.filter_weight_sum,
   N = float(spp):
       m_j      = C_j.rgb / W per channel                       (0 where W <= 0)
       lambda_j = lum(m_j) > 0 ? lum(m_j) : 0                   (so a NaN counts as no samples)
       omega_0  = 1;  for j >= 1:
           acc = 0, cnt = 0
           over the taps q = p + (dx, dy), dy = -1, 0, 1 outer, dx = -1, 0, 1 inner, those inside
           the cropped image only:
               s = (lambda_{j-1}(q) + lambda_j(q)) + lambda_{j+1}(q)     (last term omitted for j = K-1)
               acc = acc + s,  cnt = cnt + 1
           g = ((acc * N) / b_j) / cnt      the mean expected number of samples of about this
                                            brightness per neighbourhood pixel
           t = g / kappa,  omega_j = t < 1 ? t : 1              (a NaN gives 1)
       rgb   = ((m_0 + omega_1 * m_1) + omega_2 * m_2) + ...    per channel
       alpha = beauty.a / W
   The output is a nart_pixel image of totalW x totalH: cropped pixels {rgb, alpha, 1}, border pixels
   all zero, as the denoiser's; where W <= 0 the pixel is all zeros, weight included.  A non-finite
   layer pixel stays non-finite (omega * NaN), as in the beauty, and reaches no further than its own
   3x3 neighbourhood.  The image is a pure function of the inputs: no atomics, any launch shape.

   nart_hip_cascade_defaults: layers 6, start 1, base 8, kappa 2.
   nart_hip_cascade_levels (host only, no device): the K levels into levels (room for 8; null to
   query *n).  cp null: the defaults.
   nart_hip_render_cascade: renders the beauty and the K layers and reweights on the device (a
   multi-device context renders each shard's layer tiles next to its beauty tiles, gathers them with
   the beauty's gather and reweights on its first device).  image (required) receives the robust
   image; beauty, if non-null, the beauty with nart_hip_render's bits; layers, if non-null, the K layer
   images back to back (K * totalW * totalH nart_pixel), for users with their own reweighting.  cp
   null: the defaults.  The volume integrator is supported (the cascade needs no surfaces).
   nart_hip_cascade_reweight: the filter alone over host images, as nart_hip_denoise is for the
   denoiser; multi-device contexts run it on their first device.  p gives the image geometry and spp.
   nart_hip_cascade_timings: device times (ms, HIP events) of the last cascade call of the context:
   cascade_ms the split and layer splats (the slowest device's; 0 after nart_hip_cascade_reweight),
   reweight_ms the reweighting.  Either pointer may be null.
   NART_E_INVALID: layers outside 2..8, a start, base or kappa that is not finite, start <= 0,
   base <= 1, kappa <= 0, a bad level (above), a null ctx, p, image (or beauty or layers of
   nart_hip_cascade_reweight), spp < 1.  NART_E_OOM: a failed allocation; the context is then as it
   was.  Not offered: the cascade together with adaptive sampling, with the first-hit AOVs or the
   moment image, or with the denoiser in one call (there is no entry point that combines them, and
   the CLI refuses --robust with --adaptive, --aovs and --denoise); whether the robust image should
   feed the denoiser is a later decision. */
typedef struct nart_cascade_params {
    uint32_t layers;  /* K, 2..8                                                    default 6 */
    float start;      /* b_0, the first level: finite and > 0                       default 1 */
    float base;       /* the ratio between levels: finite and > 1                   default 8 */
    float kappa;      /* the neighbourhood's expected sample count at which a layer
                         is fully trusted: finite and > 0                           default 2 */
} nart_cascade_params;
void nart_hip_cascade_defaults(nart_cascade_params* cp);
int nart_hip_cascade_levels(const nart_cascade_params* cp, float* levels, uint32_t* n);
int nart_hip_render_cascade(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params* cp, nart_pixel* image,
                            nart_pixel* beauty, nart_pixel* layers, nart_render_stats* stats);
int nart_hip_cascade_reweight(nart_ctx* ctx, const nart_render_params* p, const nart_cascade_params* cp,
                              const nart_pixel* beauty, const nart_pixel* layers, nart_pixel* image);
int nart_hip_cascade_timings(const nart_ctx* ctx, double* cascade_ms, double* reweight_ms);

/* First-hit ID mattes (no reference counterpart): which mesh or material a pixel shows, and how much
   of the pixel it covers.  A filtered average of ids means nothing at a silhouette, so an id image is
   a set of (id, coverage) pairs per pixel, ranked by coverage (the Cryptomatte idea).  Opt-in: no
   other entry point changes its bits, its launches or the memory it finds; the path kernels are not
   touched.

   Id kinds.  NART_MATTE_MESH: a sample's id is the mesh index of its first-hit triangle, in scene
   order; N = num_meshes.  NART_MATTE_MATERIAL: that mesh's material index; N = num_materials.

   The first hit is exactly the first-hit AOVs' hit: the reference octree's answer at bounce 0, bounded
   by the nearest analytic light; IsectIsValid is not applied.  A miss has no id.  The feature needs
   surfaces: the volume integrator returns NART_E_UNSUPPORTED.

   Id limit.  N <= 32, because the 8 coverage planes are the extra images the frame path already
   carries; more ids return NART_E_UNSUPPORTED.  N = 0 (a scene without meshes) is allowed and gives
   empty ranks.

   Coverage planes.  There are P = ceil(N / 4) planes.  The per-sample record of plane q is
       {[id == 4q], [id == 4q+1], [id == 4q+2], [id == 4q+3]}   as 1.0f or +0.0f;
   a miss or an id >= N gives all +0.  Each plane's record stream goes through the call's splat plan and
   the tile combine exactly as Li_alpha does (the plain splat kernels, unchanged), so
   plane[q].contribution[c] is the sum of the filter weights w over the samples of id 4q+c in
   AddSample's order, and filter_weight_sum has the beauty's bits.  On the device k_matte_ids writes
   plane q's records into the per-sample record buffer once the beauty's splat (if any) has consumed
   it, once per plane per batch, each time followed by the plan's splat into that plane's tiles: no
   extra per-sample memory, as for the first-hit AOVs.

   Ranking (k_matte_rank), per pixel of the cropped image_width x image_height image (pixel (x, y) is
   total-image pixel (x + fb, y + fb)); W = plane[0].filter_weight_sum:
       c_m = plane[m / 4].contribution[m % 4] / W     one float32 divide, m < N
       only ids with c_m > 0 are candidates (zero, negative and NaN values are never ranked)
       rank r = 0 .. R-1 takes the candidate not yet taken with the greatest c_m; among equal values
       the least m wins; a rank without a candidate is {-1.0f, 0.0f}
   R = ranks: even, 2..8.
   Rank output: R / 2 nart_pixel images of totalW x totalH.  Image k holds
       {float(id_2k), c_2k, float(id_2k+1), c_2k+1, 1}
   in cropped pixels; border pixels are all zero; where W <= 0 (or with N = 0) the pixel is
   {-1, 0, -1, 0, 1}.  nart_write_exr works on these images unchanged; ids <= 31 are exact in half.

   Extraction (k_matte_extract) takes an id set as a bit mask (bit m: id m).  Per cropped pixel
       m = sum over r ascending, from 0, of c_r for the ranks whose id is in the set, in float32
   (an id is in the set when 0 <= id < 64 and bit uint(id) of the mask is set); the output is a
   nart_pixel image with cropped pixels {m, m, m, m, 1} and a zero border.

   Every output is a pure function of its inputs: no atomics, any launch shape; tests/matte_py.py
   restates planes, ranking and extraction in numpy.

   nart_hip_matte_defaults: kind mesh, ranks 6.
   nart_hip_matte_ids (host only, no device): N of a scene and kind into *n_ids; NART_E_UNSUPPORTED
   above 32 (*n_ids is still set).
   nart_hip_render_mattes: renders the P planes and ranks them on the device (a multi-device context
   renders each shard's plane tiles, gathers them with the beauty's gather and ranks on its first
   device).  ranks (required) receives the R / 2 rank images back to back; image, if non-null, the
   beauty with nart_hip_render's bits (null: a matte-only call, which launches LatinSquare, the camera
   rays and the plane passes, and no path kernel); planes, if non-null, the P plane images back to
   back.  mp null: the defaults.
   nart_hip_matte_rank: the ranking alone over P = ceil(n_ids / 4) host plane images (planes may be
   null with n_ids = 0), as nart_hip_cascade_reweight is for the cascade; nart_hip_matte_extract: the
   extraction over the R / 2 host rank images of mp.  Multi-device contexts run both on their first
   device.  p gives the image geometry.
   nart_hip_matte_timings: device times (ms, HIP events) of the last matte call of the context:
   matte_ms the plane passes (the slowest device's; 0 after nart_hip_matte_rank), rank_ms the ranking.
   Either pointer may be null.
   NART_E_INVALID: a null ctx, p, ranks or required image; an unknown kind; ranks odd or outside
   2..8; n_ids > 32 (nart_hip_matte_rank).  NART_E_UNSUPPORTED: the volume integrator, or more than 32
   ids.  An error leaves the context usable.  Not offered: the mattes together with adaptive sampling
   or the cascade in one call. */
#define NART_MATTE_MESH 0u
#define NART_MATTE_MATERIAL 1u
typedef struct nart_matte_params {
    uint32_t kind;   /* NART_MATTE_MESH or NART_MATTE_MATERIAL                      default mesh */
    uint32_t ranks;  /* R, the (id, coverage) pairs kept per pixel: even, 2..8     default 6 */
} nart_matte_params;
void nart_hip_matte_defaults(nart_matte_params* mp);
int nart_hip_matte_ids(const nart_scene_blob* scene, uint32_t kind, uint32_t* n_ids);
int nart_hip_render_mattes(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp, nart_pixel* ranks,
                           nart_pixel* image, nart_pixel* planes, nart_render_stats* stats);
int nart_hip_matte_rank(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp, uint32_t n_ids,
                        const nart_pixel* planes, nart_pixel* ranks);
int nart_hip_matte_extract(nart_ctx* ctx, const nart_render_params* p, const nart_matte_params* mp,
                           const nart_pixel* ranks, uint64_t id_mask, nart_pixel* out);
int nart_hip_matte_timings(const nart_ctx* ctx, double* matte_ms, double* rank_ms);

/* Debug / parity, as nart_hip_render_samples: the per-sample AOV records of pixels [x0,x0+w) x
   [y0,y0+h) in total-image coordinates (extra rows included) into host
   out8[((y-y0)*w + (x-x0))*spp + s][8] = albedo record then normal record; tri (optional) receives
   the first-hit triangle index or 0xFFFFFFFF.  Runs LatinSquare, the camera rays and the record
   kernel only. */
int nart_hip_render_aov_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w,
                                uint32_t h, float* out8, uint32_t* tri);

/* Edge-avoiding a-trous denoiser driven by the first-hit AOVs (no reference counterpart).

   The filter works on the cropped image_width x image_height image: pixel (x, y) is total-image
   pixel (x + fb, y + fb), fb = filter_bounds.  All arithmetic is float32 + - * / sqrt and
   comparisons, in exactly the order written here (the build contracts nothing and divides and takes
   roots correctly rounded), so that a numpy restatement (tests/denoise_py.py) gives the same bits.
   max(a, b) means a > b ? a : b and min(a, b) means a < b ? a : b; sums run in the order given,
   starting from 0.

   Prepare (k_dn_prepare), per pixel, from the beauty, albedo and normal nart_pixel images
   (contribution rgba, filter_weight_sum w):
       c    = beauty.rgba / beauty.w           (0 if beauty.w <= 0)
       a    = albedo.rgb / albedo.w, cov = albedo.a / albedo.w     (0 if albedo.w <= 0)
       hs   = albedo.a                         (sum of weight * hit)
       z    = normal.w / hs, n = normal.xyz / hs;  a pixel with hs <= 0 or z == 0 is EMPTY: n = 0, z = 0
              (no surface has depth 0; the kernels recognise an empty pixel by z == 0)
       a_d  = max(a + (1 - cov), albedo_floor) per channel      (a miss counts as albedo 1)
       s    = c.rgb / a_d;  luminance l(s) = (0.2126 s.r + 0.7152 s.g) + 0.0722 s.b
       slope = sx + sy; sx = min(|z - z_left|, |z_right - z|), at an image border the one that
              exists, 0 if the axis has one pixel; sy likewise (up, down)
   A pixel whose c.rgb has a non-finite component is INVALID: s = 0.  An invalid pixel has weight 0 as
   a tap everywhere (also as its own centre tap) and counts as variance 0 in the variance blur; as
   a centre it uses d_l = 0.  A pass that leaves it with sum(w) > 0 makes it valid with that pass's
   result; otherwise its signal stays 0 and it stays invalid.  The variance pass leaves it as it is.

   Guide terms of centre p and tap q at offset (dx, dy), cheb = max(|dx|, |dy|) (pixels, as float):
       w_n = 1 if both are empty, else min(1, max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z)),
             then w_n = w_n * w_n, normal_squarings times
       d_g = |z_p - z_q| / ((sigma_depth * (slope_p * cheb) + depth_eps * max(z_p, z_q)) + 1e-30)
             + |cov_p - cov_q| / sigma_coverage
       f(d) = t8: t = max(0, 1 - d * 0.125), t2 = t * t, t4 = t2 * t2, t8 = t4 * t4
   The centre tap of a valid pixel has w_n * f = 1.  Taps outside the image are skipped.

   Variance (k_dn_variance), 7x7, dy outer and dx inner, both ascending:
       u = w_n * f(d_g);  su += u, sl += u * l_q, sl2 += u * (l_q * l_q)
       m1 = sl / su, m2 = sl2 / su, v = max(0, m2 - m1 * m1)
   Sample variance (nart_hip_denoise_moment, nart_hip_render_denoised_moment; k_dn_prepare<true>): the
   variance comes from the second-moment image instead, and k_dn_variance does not run.  Prepare
   computes everything above, and for a valid pixel, with M the moment pixel (contribution rgba,
   filter_weight_sum mw), c and a_d as above:
       if mw > 0:  k = M.a / (mw * mw)                          (1 / the effective sample count)
                   per channel ch: m2 = M.ch / mw, var = max(0, m2 - c.ch * c.ch), V.ch = var * k
       else:       V = 0
       sd = (0.2126 * (sqrt(V.r) / a_d.r) + 0.7152 * (sqrt(V.g) / a_d.g)) + 0.0722 * (sqrt(V.b) / a_d.b)
       v  = sd * sd;  v = v < 1e30 ? v : 1e30                   (NaN and overflow become 1e30)
   V is the variance of the filtered mean per channel; no Bessel correction is applied (it is low by
   the factor 1 - k).  The channel sum takes the three channels' noise as fully correlated: the
   conservative bound, and what one light path hitting or missing produces.  An invalid pixel keeps
   v = -1 as above; the passes and finalise consume v as they do in the spatial mode.
   A-trous pass i = 0 .. iterations-1 (k_dn_atrous), step = 2^i, taps (dx, dy) = (ix, iy) * step for
   ix, iy in -2..2, iy outer, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
       vb  = sum over dy, dx in -1..1 (dy outer, coordinates clamped to the image) of
             (k[dy] * k[dx]) * max(v_q, 0), k = [1/4, 1/2, 1/4]
       d_l = |l_p - l_q| / (sigma_color * sqrt(vb) + 1e-6)
       w   = (h[ix] * h[iy]) * (w_n * f(d_g + d_l))          (centre tap: h[0] * h[0] = 9/64)
       sw += w, ss += w * s_q (per channel), sv += (w * w) * v_q
       s' = ss / sw, v' = sv / (sw * sw)
   Signal and variance ping-pong between the passes; the guides are constant.
   Finalise (k_dn_finalize): out.rgb = s * a_d, out.a = c.a (alpha passes through).

   The output is a nart_pixel image of totalW x totalH: cropped pixels {rgb, alpha, 1}, border
   pixels all zero, so nart_write_exr and contribution / filter_weight_sum work on it unchanged.
   The image is a pure function of the inputs and the parameters: no atomics, any launch shape. */
typedef struct nart_denoise_params {
    uint32_t iterations;       /* a-trous passes, 1..8: the last step is 2^(iterations-1)  default 5    */
    uint32_t normal_squarings; /* w_n = clamp(dot)^(2^normal_squarings)                    default 5    */
    float sigma_color;         /* luminance distance in standard deviations                default 4    */
    float sigma_depth;         /* depth distance in units of the local depth slope         default 1    */
    float depth_eps;           /* relative depth tolerance on flat surfaces                default 1e-3 */
    float sigma_coverage;      /* coverage distance                                        default 0.05 */
    float albedo_floor;        /* least albedo a pixel is demodulated by                   default 0.01 */
} nart_denoise_params;
void nart_hip_denoise_params_init(nart_denoise_params* dp);

/* Denoise host images: beauty, albedo and normal are nart_pixel images of totalW*totalH as
   nart_hip_render_aovs returns them (any integrator may have made the beauty), out receives the
   denoised image.  dp null: the defaults.  denoise_ms, if non-null, receives the device time of the
   denoise kernels.  Multi-device contexts run it on their first device.  NART_E_INVALID: a null
   ctx, p, image or out, iterations outside 1..8, a sigma, depth_eps or albedo_floor that is not > 0,
   normal_squarings > 16. */
int nart_hip_denoise(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                     const nart_pixel* beauty, const nart_pixel* albedo, const nart_pixel* normal, nart_pixel* out,
                     double* denoise_ms);

/* As nart_hip_denoise with the variance taken from moment, a second-moment image as
   nart_hip_render_moment returns it ("Sample variance" above); nart_hip_denoise_timings then reports
   variance_ms 0.  NART_E_INVALID additionally for a null moment or p->spp < 2 (one sample has no
   variance). */
int nart_hip_denoise_moment(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                            const nart_pixel* beauty, const nart_pixel* albedo, const nart_pixel* normal,
                            const nart_pixel* moment, nart_pixel* out, double* denoise_ms);

/* Render the beauty and both first-hit AOVs and denoise them on the device: the three images never
   pass through the host.  out receives the denoised image; image, if non-null, the noisy beauty,
   bit-identical to nart_hip_render's.  Multi-device contexts denoise on their first device after
   the gather.  Errors as nart_hip_denoise (image may be null); NART_E_UNSUPPORTED: the volume
   integrator (no first-hit AOVs).  A render without denoising launches exactly what it launched
   before. */
int nart_hip_render_denoised(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                             nart_pixel* image, nart_pixel* out, nart_render_stats* stats, double* denoise_ms);

/* As nart_hip_render_denoised in the sample-variance mode: renders the beauty, both AOVs and the
   second-moment image and denoises on the device, nothing passing through the host.  Errors as
   nart_hip_render_denoised, plus NART_E_INVALID for p->spp < 2. */
int nart_hip_render_denoised_moment(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                    nart_pixel* image, nart_pixel* out, nart_render_stats* stats, double* denoise_ms);

/* Device times (ms) of the last denoise of this context, kernel by kernel: prepare, variance, the
   a-trous passes (pass_ms[8], zero beyond the iterations run) and finalise.  Any pointer may be null. */
int nart_hip_denoise_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                             double* finalize_ms);

/* Followed guides (no reference counterpart): denoiser guides taken at the first non-delta surface.
   The first-hit AOVs of a pane of glass or a mirror show the glass or the mirror; these follow
   perfect mirrors and smooth dielectrics deterministically until something diffuse, glossy or rough
   is met, and record that surface.  Opt-in: no other entry point changes its bits, its launches or
   the memory it finds; the path kernels and the denoise kernels are not touched.

   The chain, per camera sample, draws no random numbers.  It is the path integrator's loop
   (pathintegrator.cpp:166-258) without EstimateDirect and Russian roulette, with the three
   continuation random numbers replaced by constants so that Fresnel reflection is never chosen, and
   with alphaTweak fixed at 1 (along a purely delta prefix the path's own alphaTweak is exactly 1,
   since every followed lobe reports alpha_i = 0).  All arithmetic is the path kernel's own float32
   arithmetic (path.h), operation by operation:
     state: ray = the camera ray (pinholecamera.cpp:9-40), an empty nested-dielectric list, D = 0, k = 0
     1. tmax = the nearest analytic light along ray (the light loop bound, pathintegrator.cpp:167-182);
        +inf without one.
     2. the closest hit within tmax: the reference octree's answer.  For the camera ray this is the
        first-hit AOVs' hit.
     3. no hit: the sample is a MISS, both records are all zero and the chain ends (a light met
        first is a miss, as for the first-hit AOVs).
     4. the hit's attributes (geometry.cpp:84-112) and its BSDF (Material::CreateBSDF with
        alphaTweak = 1).  t = (dot(v0, n) - dot(ray.o, n)) / dot(ray.d, n), n = cross(v1 - v0,
        v2 - v0): the plane distance exactly as the first-hit depth.  D = D + t, one float32 add, so
        D = ((t0 + t1) + t2) + ...
     5. valid = IsectIsValid(meshID, priority) of the list, which also yields eta_outer
        (pathintegrator.cpp:7-36).
     6. if valid, k < max_follow, and the BSDF has one lobe which is the perfect mirror or the
        smooth dielectric (specularbrdf.cpp, speculardielectricbrdf.cpp): wo = ToLocal(-ray.d);
        BSDF::Sample_f in its continuation form with s1 = 0 and sample = (1, 0).  sample.x = 1 is
        never < Fr, so a dielectric refracts, or reflects on total internal reflection; a mirror
        reflects.  At an index-matched interface (eta_outer == eta: Sample_f returns pdf = 0 without
        the specular flag, and the path ends there too) this hit is the guide hit.  Otherwise --
        also where total internal reflection leaves Sample_f's refraction branch with pdf = 1 - Fr
        = 0: the path, whose sample.x < 1 = Fr, takes the reflection branch there, with the same wi
        -- ray = (p + gn * 0.001 * flip, ToWorld(wi)), flip = wi.z > 0 ? 1 : -1
        (pathintegrator.cpp:216-220); a transmissive lobe updates the list with the lobe's eta; ++k,
        and go to 1.
     7. if not valid and k < max_follow: step through (pathintegrator.cpp:223-229): ray = (p + ray.d *
        0.001, ray.d), the list is updated with the eta of the lobe BSDF::Sample_f would select at
        s1 = 0; ++k, and go to 1.
     8. otherwise this hit is the GUIDE HIT:
          albedo record  {albedo.rgb, 1}, the pattern chosen by material kind as the first-hit albedo
          normal record  {normalize(n_shading).xyz, D}
   max_follow is 0..10: a chain costs at most 11 traversals, is bounded by that count and nothing
   else (a NaN direction ends it as a miss), and its list never outgrows 10 entries.  Consequences:
     - max_follow = 0 gives the first-hit AOV records bit for bit (validity is not applied to the
       hit the chain stops on);
     - a scene without mirror or smooth-glass hits gives the first-hit records bit for bit at any
       max_follow;
     - rough glass (alpha > 1e-4), glossy and plastic stop the chain.
   Both record streams go through the call's splat plan and the tile combine exactly as the first-hit
   AOVs' do, so the images have the same layout and filter_weight_sum has the beauty's bits.

   On the device k_guide (device/guide.h) traces every sample's chain once per batch after the
   beauty's splat and every other pass have consumed the per-sample record buffer: the albedo record
   goes there, the normal record into a second record buffer of 16 B per sample held for the call
   only, and only where both images are asked for (batches are then sized for 44 instead of 28 B per
   sample); then the plan's splat runs once per guide image.

   nart_hip_guide_defaults: max_follow 8.
   nart_hip_render_guides: as nart_hip_render_moment -- aovs selects the images (NART_AOV_ALBEDO,
   NART_AOV_NORMAL), which hold the followed guides; image and moment are optional, and the beauty and
   the moment image have the bits nart_hip_render / nart_hip_render_moment give.  gp null: the
   defaults.  guide_ms, if non-null, receives the device time of k_guide and the guide splats.
   Multi-device contexts gather the guide tiles with the beauty's gather.
   nart_hip_render_denoised_guides: as nart_hip_render_denoised, or with sample_variance != 0 as
   nart_hip_render_denoised_moment, the filter fed with the followed guides instead of the first-hit
   AOVs.  nart_hip_denoise / nart_hip_denoise_moment take the images of nart_hip_render_guides as they
   take any guide images, and give the same bits.
   nart_hip_render_guide_samples: debug / parity, as nart_hip_render_aov_samples: per sample i =
   ((y-y0)*w + (x-x0))*spp + s of a rect in total-image coordinates, with M = max_follow + 1,
       out8[i][8]       albedo record then normal record
       n_seg[i]         segments traced, 1..M; 0 for a camera-ray miss
       seg8[i][j][8]    {o.xyz, tmax, d.xyz, t} of segment j < max(n_seg[i], 1) (the camera ray is
                        always reported): its ray, its bound and the plane distance t of step 4
                        (tmax where the segment missed); zeros beyond
       tri[i][j]        the triangle, or 0xFFFFFFFF where that segment missed or was never traced
   seg8, tri and n_seg are optional.
   NART_E_INVALID: a null ctx, p or required image, an unknown AOV bit, a bit without its buffer,
   nothing requested, max_follow > 10, an empty or out-of-range rect; the denoise entry point also
   the errors of nart_hip_render_denoised(_moment).  NART_E_UNSUPPORTED: the volume integrator (no
   surfaces).  An error leaves the context usable.  Not offered: followed guides together with
   adaptive sampling, the cascade, the mattes, or the first-hit AOVs in one call. */
#define NART_GUIDE_MAX_FOLLOW 10u
typedef struct nart_guide_params {
    uint32_t max_follow; /* delta interfaces a chain follows or steps through, 0..10   default 8 */
} nart_guide_params;
void nart_hip_guide_defaults(nart_guide_params* gp);
int nart_hip_render_guides(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* gp, uint32_t aovs,
                           nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* moment,
                           nart_render_stats* stats, double* guide_ms);
int nart_hip_render_denoised_guides(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                    const nart_guide_params* gp, int sample_variance, nart_pixel* image,
                                    nart_pixel* out, nart_render_stats* stats, double* denoise_ms);
int nart_hip_render_guide_samples(nart_ctx* ctx, const nart_render_params* p, const nart_guide_params* gp, uint32_t x0,
                                  uint32_t y0, uint32_t w, uint32_t h, float* out8, float* seg8, uint32_t* tri,
                                  uint32_t* n_seg);

/* Half buffers: the beauty's samples split by the parity of their index into two images from a single
   render, after Rousselle, Knaus and Zwicker, "Adaptive Rendering with Non-Local Means Filtering"
   (2012), and Bitterli et al., "Nonlinearly Weighted First-order Regression for Denoising Monte Carlo
   Renderings" (2016).  Two images of independent halves of the samples are what cross-filtering
   denoisers and error estimates start from: the difference of the halves estimates the noise of their
   average without assuming independent samples within a pixel (ours are Latin-square stratified).

   Half image h (0 or 1), a nart_pixel image laid out as the beauty:
       contribution      { sum w r, sum w g, sum w b, sum w } over the (sample, pixel) pairs of the
                         beauty's splat whose sample index i has i mod 2 == h, in the beauty's order
       filter_weight_sum the beauty's: sum w over all samples, with the beauty's bits
   i is the sample's index 0..spp-1 in its pixel's sequence: the s of nart_hip_render_samples.  The
   half's mean is rgb / contribution[3], normalised by its own weights; finalize and the EXR writer
   divide by filter_weight_sum as for any image, so that the two written halves add up to the beauty
   up to rounding.  At spp 1 half 0 has the beauty's rgb bits and half 1 is zero but for
   filter_weight_sum.

   On the device k_half_split (device/halves.h) runs once per half per batch after the beauty's splat
   and before any other pass overwrites the per-sample records: a sample of parity h writes
   {L.r, L.g, L.b, 1} (the colour copied: a non-finite colour reaches exactly one half), every other
   sample {0, 0, 0, 0}, into a second record buffer of 16 B per sample held for the call only; the
   plan's splat then takes it into the half's tiles, unchanged (adding the zero records changes no
   bit of a finite sum).

   nart_hip_render_halves: image, half_a (h = 0) and half_b (h = 1) are required; aovs selects the
   albedo and normal images (NART_AOV_ALBEDO, NART_AOV_NORMAL) as nart_hip_render_aovs does, and with
   gp non-null they hold the followed guides of nart_hip_render_guides.  The beauty, the AOVs and the
   guides have the bits those entry points give.  halves_ms, if non-null, receives the device time of
   the splits and the half splats.  The volume integrator is supported where aovs is 0.  Multi-device
   contexts gather the half tiles with the beauty's gather.
   NART_E_INVALID: a null ctx, p, image, half_a or half_b, an unknown AOV bit, a bit without its
   buffer, max_follow > 10.  NART_E_UNSUPPORTED: AOVs or guides with the volume integrator.  An error
   leaves the context usable.  Not offered: half buffers together with the moment image, adaptive
   sampling, the cascade, the mattes, light groups, depth cuts or the cost image in one call. */
int nart_hip_render_halves(nart_ctx* ctx, const nart_render_params* p, uint32_t aovs, const nart_guide_params* gp,
                           nart_pixel* image, nart_pixel* albedo, nart_pixel* normal, nart_pixel* half_a, nart_pixel* half_b,
                           nart_render_stats* stats, double* halves_ms);

/* Cross-filtered denoising: the a-trous denoiser above over the two half buffers, each half filtered
   with colour weights taken from the other half, after Rousselle et al. 2012 and Bitterli et al. 2016
   (see "Half buffers").  The plain denoiser compares lum(s_p) and lum(s_q) of the signal it averages:
   a pixel that is bright by chance rejects its neighbours and survives.  Here the noise of the
   weights is independent of the noise they average, and the difference of the two filtered halves
   estimates the error of their average.

   Everything is float32 + - * / sqrt and comparisons in the order below, built without contraction;
   tests/denoise_cross_py.py restates it.  Sums start at 0 and run over dy then dx, ascending, as the
   plain denoiser's do; min, max, lum, the guide terms w_n, d_g and the falloff f are the plain
   denoiser's ("Guide terms").  H_h is half image h, p a pixel of the cropped window.

   Prepare.  The guide {n, z}, the coverage, a_d, the depth slope and alpha are what the plain
   denoiser's prepare computes from the albedo, normal and beauty images.
       c_h = H_h.rgb / H_h[3]                 per half, by its own weight sum
       valid(p): H_0[3] > 0 and H_1[3] > 0 and all six components of c_0, c_1 finite
       s_h = c_h / a_d                         per channel
       d   = lum(s_0) - lum(s_1)
       v   = 0.5f * (d * d)                    the initial variance of both halves
   v is the one-sample estimate of the variance of one half's luminance (the two halves have equal
   variance and d has twice it), so that den = sigma_color * sqrt(v) stands against a tap difference
   of variance 2 v as in the plain denoiser.  An invalid pixel is {0, 0, 0, -1} in both halves.

   Variance.  For a valid p, over the taps q of the 7x7 window that lie in the image and are valid:
       u = 1 at the centre, else w_n * f(d_g + 0)
       su = su + u;  sv = sv + u * v(q)        v(p) <- sv / su, for both halves
   An invalid pixel stays as it is.

   A-trous pass at step 2^i, for every p (valid or not), both halves at once.  With o = 1 - h:
       vb_h   = sum over the 3x3 taps (clamped coordinates) of k * max(v_h(q), 0), k = {1/4, 1/2, 1/4}^2
       den_h  = sigma_color * sqrt(vb_o) + 1e-6f, lp_h = lum(s_o(p))     where half o is valid at p
   For each tap q = p + step * (ix, iy), ix, iy in -2..2, inside the image, with a valid half:
       (w_n, d_g) once per tap, with cheb = step * max(|ix|, |iy|)       (not at the centre)
       for h = 0, 1 where half h is valid at q:
           d_l = |lp_h - lum(s_o(q))| / den_h   where half o is valid at p and at q, else 0
           w   = h_x * h_y at the centre, else (h_x * h_y) * (w_n * f(d_g + d_l))
           sw_h += w;  s_h' += w * s_h(q) per channel;  sv_h += (w * w) * v_h(q)
       s_h(p) <- s_h' / sw_h,  v_h(p) <- sv_h / (sw_h * sw_h)     where sw_h > 0, else half h is invalid at p
   The colour distance of half h comes from the other half, and den_h from the variance of the half
   whose colours are compared.

   Finalize.  Cropped pixels, per channel c:
       out_c = ((s_0c + s_1c) * 0.5f) * a_d_c                         out   = {out.rgb, alpha, 1}
       t     = ((s_0c - s_1c) * 0.5f) * a_d_c;  e_c = t * t           error = {e.rgb, alpha, 1}
   A pixel with an invalid half gets the beauty's mean (0 where its weight sum is <= 0) and error 0.
   Border pixels are zero in both images.  e_c is a one-degree-of-freedom estimate per pixel of the
   squared error of out_c: average it over a neighbourhood before use.

   The order is symmetric in the halves: + and * commute, d and t only change sign before they are
   squared, and each half's sums see the other half's values in the same places.  Swapping half_a and
   half_b leaves both images bit-equal.  With identical halves d = 0 and v = 0 throughout, s_0 = s_1,
   the error is exactly 0 and out.rgb has the bits of the plain denoiser's prepare, a-trous passes
   and finalise run with variance 0 (no variance kernel) on a beauty whose mean is the halves'.

   On the device (device/denoise_cross.h) k_dnx_prepare, k_dnx_variance, k_dnx_atrous<R> and
   k_dnx_finalize run on 32 x 8 tiles with the plain denoiser's LDS halo scheme (two signals, one
   guide and the coverage per staged pixel: 52 B, at most 40 x 16 pixels); the guide half of a tap
   weight is computed once for both halves.

   nart_hip_denoise_cross: host images in, as nart_hip_denoise: the two halves and the beauty of
   nart_hip_render_halves, the albedo and normal images (first-hit or followed); out receives the
   denoised image and error, if non-null, the error image.  dp null: the defaults of
   nart_hip_denoise_params_init, which are not changed.  denoise_ms: the device time.
   nart_hip_render_denoised_cross: renders the halves and the AOVs (gp non-null: the followed
   guides) and filters them on the device; nothing but out, error and, if non-null, image (the beauty)
   passes the host.  The images equal nart_hip_denoise_cross fed with nart_hip_render_halves' images.
   nart_hip_denoise_cross_timings: as nart_hip_denoise_timings, of the last cross call.
   NART_E_INVALID: a null ctx, p or required image, p->spp < 2 (a half would be empty), the parameter
   errors of nart_hip_denoise, max_follow > 10.  NART_E_UNSUPPORTED (nart_hip_render_denoised_cross):
   the volume integrator (the guides need surfaces).  An error leaves the context usable. */
int nart_hip_denoise_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, const nart_pixel* half_a,
                           const nart_pixel* half_b, const nart_pixel* beauty, const nart_pixel* albedo,
                           const nart_pixel* normal, nart_pixel* out, nart_pixel* error, double* denoise_ms);
int nart_hip_render_denoised_cross(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                   const nart_guide_params* gp, nart_pixel* out, nart_pixel* error, nart_pixel* image,
                                   nart_render_stats* stats, double* denoise_ms);
int nart_hip_denoise_cross_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                                   double* finalize_ms);

/* Light groups: the beauty split by light, one image per group of lights from a single render, so
   that a light can be dimmed, tinted or switched off afterwards (nart_hip_light_mix) without tracing
   a path again.

   In PathIntegrator::Li_alpha radiance enters a sample's L at two places only: L += EstimateDirect(...)
   * beta, whose two MIS terms both come from the one light the call drew, and L = Le of the one light
   a camera ray escapes to.  Every term of L therefore belongs to exactly one light, and no RNG draw,
   pdf, hit or alpha depends on a light's emission.

   Inputs: group_of_light[n_lights], one entry per light of the scene in scene order, each < n_groups;
   1 <= n_groups <= NART_LIGHT_GROUPS_MAX.
   Per camera sample and group g the group record is {Lg.r, Lg.g, Lg.b, alpha}:
     1. alpha is the sample's beauty alpha;
     2. Lg starts at +0 and receives, in path order, exactly the terms the beauty's L receives whose
        light is in group g, by the same operation: Lg = Lg + mul(muls(Led, numLights), beta_k) for a
        shaded hit whose EstimateDirect drew a light of g (Led = ((0 + c1) + c2) over the unoccluded
        terms, zero terms included), and Lg = Le when the camera ray escapes to a light of g (an
        assignment, as in the reference);
     3. terms of other groups are skipped, not multiplied by zero.
   The group image is these records through the call's unchanged splat and tile combine: a full
   nart_pixel image whose alpha and filter_weight_sum have the beauty's bits.
   It is bit-identical to a render of the scene with every other light's intensity set to 0 wherever
   that render forms no 0 * inf: there a zero-intensity light's term is 0 * numLights * beta_k, which is
   +-0 (and leaves L's bits alone) unless beta_k is infinite or NaN, where it is NaN and the group image
   is not.  A group image's own NaNs and infinities are the beauty's.  One group holding every light
   gives the beauty bit for bit.

   Mix: out = mix(groups, gains[n_groups][3]) over the totalW x totalH image; per pixel and channel c
   of r, g, b:  acc = 0.f; for g ascending: acc = acc + gains[g][c] * I_g.contribution[c]  (float32,
   unfused, in this order); alpha and filter_weight_sum are copied from I_0.  Gains must be finite.

   On the device a light-group build of the ray-queue path kernel (k_render_rq with LG: the generic
   two-wave build without priority lanes or speculative pairs, which hold a sample's result pending
   and may drop it; small shards of a group frame run the plain schedule) accumulates the records in G
   record arrays in global memory, 16 B per sample and group, held for the call (batches are sized for
   28 + 16 G bytes per sample); the plan's splat then runs once per group, and k_light_mix
   (device/lightgroup.h) mixes, one lane per pixel.  The counter pass has no light-group build: with
   nart_hip_set_counters enabled a light-group render reports no work counts.

   nart_hip_render_light_groups: groups receives the n_groups images back to back (required); image,
   if non-null, the beauty, with the bits nart_hip_render gives.  Multi-device contexts gather the
   group tiles with the beauty's gather.
   nart_hip_light_mix: groups holds n_groups host images back to back; out receives the mix.
   nart_hip_render_light_group_samples: debug / parity, as nart_hip_render_samples: the group records
   of a rect in total-image coordinates into out[g][((y-y0)*w + (x-x0))*spp + s][4].
   nart_hip_light_group_timings: device times of the last call's group splats and of the last mix.
   NART_E_INVALID: a null ctx, p, map, groups, gains or out; n_groups outside 1..8; a map whose length
   is not the scene's light count or that holds a value >= n_groups; a gain that is not finite; an
   empty or out-of-range rect.  NART_E_UNSUPPORTED: the volume integrator; variant 3 or a BVH deeper
   than the ray-queue kernel's LDS holds (k_render has no light-group build).  An error leaves the
   context usable.  Not offered: light groups together with adaptive sampling, the cascade, the
   mattes, AOVs, guides, the moment image or the denoiser in one call. */
#define NART_LIGHT_GROUPS_MAX 8u
int nart_hip_render_light_groups(nart_ctx* ctx, const nart_render_params* p, const uint32_t* group_of_light,
                                 uint32_t n_lights, uint32_t n_groups, nart_pixel* groups, nart_pixel* image,
                                 nart_render_stats* stats);
int nart_hip_light_mix(nart_ctx* ctx, const nart_render_params* p, uint32_t n_groups, const float* gains,
                       const nart_pixel* groups, nart_pixel* out);
int nart_hip_render_light_group_samples(nart_ctx* ctx, const nart_render_params* p, const uint32_t* group_of_light,
                                        uint32_t n_lights, uint32_t n_groups, uint32_t x0, uint32_t y0, uint32_t w,
                                        uint32_t h, float* out);
int nart_hip_light_group_timings(const nart_ctx* ctx, double* splat_ms, double* mix_ms);

/* Depth cuts: the image at lower bounce limits from a single render -- direct against indirect light,
   what the third bounce still adds, the limit at which the picture stops changing.

   Lowering p->bounces and rendering again does not give that split.  A pixel's samples share one RNG
   stream (RenderTile seeds once per pixel and hands the same rng to every Li_alpha), so a render with
   a lower limit draws fewer numbers per sample and traces different paths from each pixel's second
   sample on: "beauty minus a direct-only render" carries the noise of two renders and goes negative.
   The cut images of one render share their paths.

   Inputs: cuts[n_cuts], 1 <= n_cuts <= NART_DEPTH_CUTS_MAX, strictly ascending, 1 <= cuts[j] <=
   p->bounces.  Per camera sample and cut d the record is {L_d.r, L_d.g, L_d.b, alpha}:
     1. L_d holds the bits of L in PathIntegrator::Li_alpha at the moment its loop counter `bounce`
        first equals d;
     2. if the loop ends sooner -- by a miss, the bounce == 0 escape with L = Le, scatteringPdf <= 0,
        roulette, or the limit -- L_d is the final L;
     3. a stepped-through lower-priority interface is a bounce without a term;
     4. alpha is the sample's alpha.  It is settled at bounce 0: the dielectric list is empty at the
        camera, so a first hit is always valid.
   A cut image is these records through the call's unchanged splat and tile combine: a full nart_pixel
   image whose alpha and filter_weight_sum have the beauty's bits.  cuts[j] == p->bounces gives the
   beauty bit for bit.  Per sample the records never decrease with the depth (every term is
   non-negative and float addition is monotone), and the differences of neighbouring cut images are the
   light each range of bounces added.

   Yardstick: L_d is the result of the same loop stopped at d, started from the same RNG state, so a
   render with bounces = d agrees exactly where the start state agrees: the whole frame at spp = 1, and
   the first sample of every pixel at any spp.  Later samples of a pixel are not comparable to any
   render with another bounce limit.

   Layers: layers(cut_images[K], beauty) gives K + 1 images over the totalW x totalH image; per pixel
   and channel of r, g, b:  layer_0 = I_0;  layer_j = I_j - I_{j-1};  layer_K = beauty - I_{K-1};  each
   one float32 subtraction.  Alpha and filter_weight_sum are copied from the beauty.  With cuts = {1}
   the layers are direct and indirect light.

   On the device a depth-cut build of the ray-queue path kernel (k_render_rq with DC: the generic
   two-wave build without priority lanes or speculative pairs, as for light groups) writes the records
   into K record arrays in global memory, 16 B per sample and cut (batches are sized for 28 + 16 K
   bytes per sample): the record of the cut equal to the kernel's bounce count where a bounce's
   EstimateDirect term has been added, every deeper cut where the sample ends.  The plan's splat then
   runs once per cut, and k_depth_layers (device/depthcut.h) subtracts, one lane per pixel.  The
   counter pass has no depth-cut build.

   nart_hip_render_depth_cuts: cut_images receives the n_cuts images back to back (required); image, if
   non-null, the beauty, with the bits nart_hip_render gives.  Multi-device contexts gather the cut
   tiles with the beauty's gather.
   nart_hip_depth_layers: cut_images holds n_cuts host images back to back, beauty one; out receives
   the n_cuts + 1 layers back to back.
   nart_hip_render_depth_cut_samples: debug / parity, as nart_hip_render_samples: the cut records of a
   rect in total-image coordinates into out[j][((y-y0)*w + (x-x0))*spp + s][4].
   nart_hip_depth_cut_timings: device times of the last call's cut splats and of the last layers run.
   NART_E_INVALID: a null ctx, p, cuts, cut_images, beauty or out; n_cuts outside 1..8; cuts that are
   not strictly ascending; a cut of 0 or above p->bounces; an empty or out-of-range rect.
   NART_E_UNSUPPORTED: the volume integrator; variant 3 or a BVH deeper than the ray-queue kernel's LDS
   holds (k_render has no depth-cut build).  An error leaves the context usable.  Not offered: depth
   cuts together with adaptive sampling, the cascade, the mattes, AOVs, guides, the moment image, light
   groups or the denoiser in one call (the layers are denoised separately, with shared guides, by
   nart_hip_render_denoised_depth_layers and nart_hip_denoise_parts: "Denoised parts" below). */
#define NART_DEPTH_CUTS_MAX 8u
int nart_hip_render_depth_cuts(nart_ctx* ctx, const nart_render_params* p, const uint32_t* cuts, uint32_t n_cuts,
                               nart_pixel* cut_images, nart_pixel* image, nart_render_stats* stats);
int nart_hip_depth_layers(nart_ctx* ctx, const nart_render_params* p, uint32_t n_cuts, const nart_pixel* cut_images,
                          const nart_pixel* beauty, nart_pixel* out);
int nart_hip_render_depth_cut_samples(nart_ctx* ctx, const nart_render_params* p, const uint32_t* cuts, uint32_t n_cuts,
                                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, float* out);
int nart_hip_depth_cut_timings(const nart_ctx* ctx, double* splat_ms, double* layers_ms);

/* Denoised parts: the light groups or the depth layers of a render, each denoised on its own, with one
   set of guides for all of them (no reference counterpart).

   A group image that is re-gained in comp is as noisy as the beauty was, and direct light (hard shadow
   edges, low variance) and indirect light (smooth, noisy) want different luminance weights: one
   variance for their sum blurs the edge or keeps the noise.  So the parts are denoised one by one.

   Definition: n_parts part images, 1 <= n_parts <= NART_DENOISE_PARTS_MAX (8 light groups, or the 9
   layers of 8 depth cuts), one albedo and one normal image.  For every k, out[k] has the bits of
   nart_hip_denoise over (parts[k], albedo, normal) with the same parameters: the filter above run on
   part k alone.  That holds for every n_parts, every chunking (below), every image size, and for pixels
   that are invalid, empty or outside the crop; a pixel may be invalid in one part and valid in another.
   Only the spatial variance estimate is offered: the sample-variance mode would need a second-moment
   image per part.

   Factorisation: the weight of a tap is w_n * f(d_g + d_l) ("Guide terms" above), and w_n and d_g -- the
   normal dot product and its squarings, the depth division, the coverage division -- are the guides'
   alone.  The kernels (device/denoise_parts.h) prepare guide, cov, slope and a_d once, and signal, alpha
   and validity per part; a launch then takes a chunk of 1..4 parts, computes w_n and d_g once per tap,
   and per part d_l, f, the weight and the sums, with the operations and the order written above.  In
   the variance pass u = w_n * f(d_g) is shared and su, sl, sl2 are per part, because an invalid tap is
   skipped per part.  NART_DN_PARTS_CHUNK = 1..4 forces the chunk size (0 or unset: the measured choice
   per n_parts, host/denoise_parts_plan.h); it changes no bit.

   Sum: per pixel of the total image and channel of r, g, b,  sum = ((out_0 + out_1) + out_2) + ...  in
   float32, starting from out_0 itself (no 0 is added, so -0 stays); alpha and filter_weight_sum are
   out_0's.

   nart_hip_denoise_parts: host images; parts and out hold n_parts images back to back; sum, if non-null,
   receives the sum.  One upload, the stage, one download.  denoise_ms: the device time of the stage.
   nart_hip_render_denoised_light_groups: as nart_hip_render_light_groups, and denoises the n_groups group
   images: denoised receives them back to back (required); optional: sum, their sum; groups, the noisy
   group images; image, the noisy beauty -- these two with the bits nart_hip_render_light_groups gives.
   nart_hip_light_mix takes the denoised groups unchanged.
   nart_hip_render_denoised_depth_layers: as nart_hip_render_depth_cuts, then the n_cuts + 1 layers on the
   device, and denoises them: denoised receives them back to back (required); optional: sum; layers, the
   noisy layers, with the bits of nart_hip_depth_layers over nart_hip_render_depth_cuts; image, the beauty.
   gp null: the first-hit AOVs are the guides; non-null: the followed guides, as
   nart_hip_render_denoised_guides.
   Both whole-frame calls render two frames of the existing kinds back to back -- the light-group or
   depth-cut frame, then a frame without beauty that asks for both AOVs (or both followed guides): camera
   rays only, no path kernel -- into device images of the first device, and run the stage there; nothing
   but what the caller asked for passes the host.  All device images and work buffers are temporaries of
   the call.  stats describe the first frame and the stage; multi-device contexts gather as before and
   denoise on their first device.
   nart_hip_denoise_parts_timings: device times (ms) of the last parts denoise, kernel by kernel and
   summed over the chunks: prepare, variance, the passes (pass_ms[8]), finalise, the sum; and guides_ms,
   the render_ms of the last whole-frame call's guides frame.  Any pointer may be null.
   NART_E_INVALID: a null ctx, p or required image; n_parts outside 1..9; whatever nart_hip_denoise,
   nart_hip_render_light_groups, nart_hip_render_depth_cuts and nart_guide_params reject.
   NART_E_UNSUPPORTED: the volume integrator; what the light-group and depth-cut builds refuse.  An error
   leaves the context usable. */
#define NART_DENOISE_PARTS_MAX 9u
int nart_hip_denoise_parts(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp, uint32_t n_parts,
                           const nart_pixel* parts, const nart_pixel* albedo, const nart_pixel* normal, nart_pixel* out,
                           nart_pixel* sum, double* denoise_ms);
int nart_hip_render_denoised_light_groups(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                          const nart_guide_params* gp, const uint32_t* group_of_light, uint32_t n_lights,
                                          uint32_t n_groups, nart_pixel* denoised, nart_pixel* sum, nart_pixel* groups,
                                          nart_pixel* image, nart_render_stats* stats, double* denoise_ms);
int nart_hip_render_denoised_depth_layers(nart_ctx* ctx, const nart_render_params* p, const nart_denoise_params* dp,
                                          const nart_guide_params* gp, const uint32_t* cuts, uint32_t n_cuts,
                                          nart_pixel* denoised, nart_pixel* sum, nart_pixel* layers, nart_pixel* image,
                                          nart_render_stats* stats, double* denoise_ms);
int nart_hip_denoise_parts_timings(const nart_ctx* ctx, double* prepare_ms, double* variance_ms, double* pass_ms,
                                   double* finalize_ms, double* sum_ms, double* guides_ms);

/* Cost image: per-pixel ray, hit and traversal counts of a render -- where its time goes.

   A shard's time is set by its costliest pixels' serial sample chains; the whole-frame totals of the
   counter pass (nart_hip_set_counters) do not say where those pixels are.  For every traced camera
   sample the cost record is four uint32 (nart_cost_pixel):
     rays_extend  closest-hit queries of the sample, as nart_render_stats::rays_extend: the camera ray
                  when p->bounces > 0, plus one per continued bounce;
     rays_shadow  occlusion queries of EstimateDirect actually traced, as nart_render_stats::rays_shadow
                  (the device skips a query whose term is exactly zero);
     hits         shaded hits, as nart_render_stats::bounces;
     steps        BVH node visits plus triangle tests of the sample's own extension and shadow rays, as
                  nart_render_stats::node_visits + tri_tests count them, from the start of a ray's
                  traversal until it resolves, whichever lane traces it.
   The cost grid is the sum of a pixel's records over its p->spp samples, (grid_h, grid_w) nart_cost_pixel,
   on the grid of traced pixels: grid_w = min(bucket_size * n_buckets_x, total_width), grid_h likewise --
   the x, y range of RenderTile's loops, the rows and columns beyond the cropped window included
   (nart_hip_cost_grid).  grid_w * grid_h * spp is nart_render_stats::traced_samples.  Per sample:
   1 <= rays_extend <= bounces (bounces > 0), rays_extend - 1 <= hits <= rays_extend, rays_shadow <= 2 hits.

   Every word depends on the scene and the session only, not on the schedule.  A cost frame runs the
   cost build of the ray-queue path kernel (k_render_rq with CS: the generic two-wave build without
   priority lanes or speculative pairs, as for light groups and depth cuts, so no traced work is
   dropped) and no k_primary: the camera rays are traced by the path kernel too, so every ray of a
   sample goes through the single-ray traversal and packet traversal, whose steps are a wave's union,
   never enters `steps`.  The owning lane writes one 16-byte record per sample (batches are sized for
   28 + 16 bytes per sample); k_cost_reduce (device/cost.h) sums a slot's records into the grid once per
   batch.  The beauty of a cost render has the bits nart_hip_render gives.  With nart_hip_set_counters
   enabled a cost render reports no work counts: the grid holds them.

   nart_hip_cost_grid: the grid's size for p; host only.
   nart_hip_render_cost: cost receives the grid (required); beauty, if non-null, the beauty.  On a
   multi-device context every device reduces its own buckets into its own zeroed grid and the host adds
   them: each pixel is non-zero on exactly one device.
   nart_hip_render_cost_samples: debug / parity, as nart_hip_render_samples: the records of a rect in
   total-image coordinates (which are the grid's) into records[((y-y0)*w + (x-x0))*spp + s][4].
   nart_hip_cost_image: a grid as a nart_pixel image the EXR writer and finalize() take unchanged: grid
   pixel (x, y) goes to image pixel (y + fb, x + fb) as {float(rays_extend), float(rays_shadow),
   float(hits), float(steps), float(spp)} (round to nearest even); grid pixels outside the total image
   are dropped and the rest of the image is zero, so finalize() gives per-sample means over the cropped
   window.
   nart_hip_cost_timings: device times of the last cost render's reduces and of the last image run.
   NART_E_INVALID: a null ctx, p, cost, image or records; an empty or out-of-range rect.
   NART_E_UNSUPPORTED: the volume integrator; variant 3 or a BVH deeper than the ray-queue kernel's LDS
   holds (k_render has no cost build).  An error leaves the context usable.  Not offered: the cost image
   together with adaptive sampling, the cascade, the mattes, AOVs, guides, the moment image, light groups,
   depth cuts or the denoiser in one call. */
typedef struct nart_cost_pixel { uint32_t rays_extend, rays_shadow, hits, steps; } nart_cost_pixel;
int nart_hip_cost_grid(const nart_render_params* p, uint32_t* width, uint32_t* height);
int nart_hip_render_cost(nart_ctx* ctx, const nart_render_params* p, nart_cost_pixel* cost, nart_pixel* beauty,
                         nart_render_stats* stats);
int nart_hip_render_cost_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0, uint32_t w,
                                 uint32_t h, uint32_t* records);
int nart_hip_cost_image(nart_ctx* ctx, const nart_render_params* p, const nart_cost_pixel* cost, nart_pixel* image);
int nart_hip_cost_timings(nart_ctx* ctx, double* reduce_ms, double* image_ms);

/* Multi-GPU building block: render the listed buckets (bucket id = by*nBucketsX + bx) into
   device-resident tiles d_tiles[i] (tile_size^2 nart_pixel each, same order as the list) on
   `stream` (a hipStream_t, may be 0).  bucket_ids is a host array.  Asynchronous w.r.t. the
   host except for small scratch uploads; synchronise the stream before reading d_tiles. */
int nart_hip_render_buckets_async(nart_ctx* ctx, const nart_render_params* p,
                                  const uint32_t* bucket_ids, uint32_t n_buckets,
                                  nart_pixel* d_tiles, void* stream, nart_render_stats* stats);

/* Device combine: d_tiles indexed by bucket id (all nBucketsX*nBucketsY tiles) into the
   totalW*totalH device image, bucket raster order (render.cpp:183-203). */
int nart_hip_combine_async(nart_ctx* ctx, const nart_render_params* p, const nart_pixel* d_tiles,
                           nart_pixel* d_image, void* stream);

/* Debug / parity: per-sample Li_alpha (float4) for pixels [x0,x0+w) x [y0,y0+h) in image
   coordinates, all spp samples, into host out[((y-y0)*w + (x-x0))*spp + s][4]. */
int nart_hip_render_samples(nart_ctx* ctx, const nart_render_params* p, uint32_t x0, uint32_t y0,
                            uint32_t w, uint32_t h, float* out);

/* Enable the deterministic counter pass (node visits, triangle tests, rays) for the next
   renders.  Slower; used to compute algorithmic bytes per sample. */
int nart_hip_set_counters(nart_ctx* ctx, int enable);

/* Device self-test: glibc-equivalent sinf/cosf over n inputs (parity of the device libm).  The
   general entry is nart_hip_eval (NART_EVAL_SINCOS computes the same values). */
int nart_hip_eval_sincos(nart_ctx* ctx, const float* x, uint32_t n, float* sin_out, float* cos_out);

/* Device probe (test hook, never launched by a render): one device function of the render path
   on n caller-supplied inputs, one lane per input.  in and out hold n records of NART_EVAL_WORDS
   (16) floats each; integer fields (u32) travel as their bits; input words an op does not name are
   ignored and output words it does not name are 0.

     op                       in                                        out
     ACOSF ATANF LOGF         0 x                                       0 f(x)
     LOGF_LDS                 0 x     (logf through the volume kernel's LDS table)   0 logf(x)
     ATAN2F                   0 y, 1 x                                  0 atan2f(y, x)
     SINCOS                   0 x                                       0 sinf(x), 1 cosf(x)
     F2U32 F2U8               0 f                                       0 u32 result
     GMOD                     0 a, 1 b                                  0 a - b * floor(a / b)
     GFRACT                   0 x                                       0 x - floor(x)
     RNG_FLOAT                0 u32 state                               0 value, 1 u32 state after
     RNG_INT                  0 u32 state, 1 u32 max                    0 u32 value, 1 u32 state after
     SAMPLE_DISK              0-1 sample                                0-1 point
     SAMPLE_RING              0-1 sample, 2 inner                       0-1 point, 2 pdf
     SAMPLE_COSHEMI           0-1 sample                                0-2 direction, 3 pdf
     SAMPLE_SPHERE            0-1 sample                                0-2 direction
     SAMPLE_WH                0-1 sample, 2 alpha, 3 u32 diel (0/1), 4-6 wo      0-2 wh
     FRESNEL                  0 eta_o, 1 eta_i, 2 cos_theta             0 Fr
     BXDF_F                   shading record, 12-14 wi                  0-2 f
     BXDF_PDF                 shading record, 12-14 wi                  0 pdf
     BXDF_F_PDF               shading record, 12-14 wi                  0-2 f, 3 pdf
     BXDF_SAMPLE_F            shading record, 12 s1, 13-14 sample       0-2 f, 3-5 wi, 6 pdf, 7 u32 flags,
                                                                        8 alpha_i (-1 where not written)

   Shading record: 0 u32 packed = type (bits 0-7: 0 Lambert, 1 specular, 2 specular dielectric,
   3 dielectric, 4 Torrance-Sparrow) | uap << 8 (use alpha_prime) | incoming flags << 16 (8 bits, the
   reference's uint8_t; BXDF_SAMPLE_F only); 1-3 rho; 4 tau (the lobe's tau is (tau, tau / 2, tau / 4):
   three distinct channels from one word); 5 eta; 6 alpha_0; 7 alpha_prime; 8 eta_outer; 9-11 wo.

   fm: the path kernel's feature mask (NART_FT_*) that BXDF_F_PDF and BXDF_SAMPLE_F are compiled
   for: NART_FT_ALL, or one of NART_FT_LAMBERT, _SPECULAR, _GLASS, _GLOSSY, _PLASTIC (per BxDF kind
   the narrowest mask that creates it; give such a build only the kinds its mask creates).  The other
   ops ignore the build but fm must still be one of these.
   NART_E_INVALID: a null pointer, an unknown op, any other fm, n above NART_EVAL_MAX_N (1 GiB of
   records each way; the block count stays far from 32 bits).  n == 0: NART_OK, nothing launched.
   Multi-device contexts run it on their first device. */
#define NART_EVAL_WORDS 16
#define NART_EVAL_MAX_N (1u << 24)
enum {
    NART_EVAL_ACOSF = 0, NART_EVAL_ATANF = 1, NART_EVAL_ATAN2F = 2, NART_EVAL_LOGF = 3, NART_EVAL_LOGF_LDS = 4,
    NART_EVAL_SINCOS = 5, NART_EVAL_F2U32 = 6, NART_EVAL_F2U8 = 7, NART_EVAL_GMOD = 8, NART_EVAL_GFRACT = 9,
    NART_EVAL_RNG_FLOAT = 10, NART_EVAL_RNG_INT = 11, NART_EVAL_SAMPLE_DISK = 12, NART_EVAL_SAMPLE_RING = 13,
    NART_EVAL_SAMPLE_COSHEMI = 14, NART_EVAL_SAMPLE_SPHERE = 15, NART_EVAL_SAMPLE_WH = 16, NART_EVAL_FRESNEL = 17,
    NART_EVAL_BXDF_F = 18, NART_EVAL_BXDF_PDF = 19, NART_EVAL_BXDF_F_PDF = 20, NART_EVAL_BXDF_SAMPLE_F = 21,
    NART_EVAL_N_OPS = 22
};
int nart_hip_eval(nart_ctx* ctx, uint32_t op, uint32_t fm, const float* in, uint32_t n, float* out);

/* Device trace probe (test hook, never launched by a render): n caller-supplied rays against the
   context's own device scene (its BVH, permuted triangle records and octree tables), each answered by
   one of the render kernels' traversal entry points, one lane per ray, 256-lane blocks.

   in: n records of NART_TRACE_IN_WORDS (8) words: 0-2 origin, 3 tmax, 4-6 direction (used as given,
   not normalised), 7 u32 query kind (NART_TRACE_CLOSEST, NART_TRACE_ANY).
   out: n records of NART_TRACE_OUT_WORDS (32) u32 words:
     0      closest: the winning scene triangle or NART_TRACE_NO_HIT; any: 1 (a hit exists) or 0
     1      closest: the bits of t (tmax on a miss); any: 0
     2-5    with count != 0 the lane's TraceCounters: nodes, triangle tests, exact octree ancestor
            checks, octree replays; else 0
     6-25   closest hit only (else 0): the Isect that fill_isect produces, as float bits: 6-8 p,
            9-11 gn, 12-14 sn, 15-17 dpds, 18-20 dpdt, 21-22 st; u32 23 meshID, 24 priority, 25 material
     26-31  0

   variant: which entry point answers.
     NART_TRACE_PLAIN     traverse<>, no node in LDS (k_guide, k_primary's per-lane form); LDS: their stack
     NART_TRACE_LDS       traverse<> over the top nodes staged by stage_nodes (k_render); LDS: k_render's layout
     NART_TRACE_STEP      trav_begin / trav_step / oc_resolve as k_render_rq runs them, nodes staged
     NART_TRACE_STEP_ROT  ... with the rotated node quarters of the environment-light builds
     NART_TRACE_PACKET    traverse_packet, one wave per 64 consecutive records (closest queries only;
                          the last wave may be partial); LDS: k_primary_px's wave stacks
   sk (the STEP variants; the others ignore it): 0 = the whole stack in LDS (the two-wave builds); 1 ..
   stack_depth = the lean build's short stack, sk levels in LDS and the rest in a per-thread global
   column.  The staged node count is what a 256-lane ray-queue block with that stack would stage.

   NART_E_INVALID: a null pointer, an unknown variant, sk above the context's stack depth, n above
   NART_EVAL_MAX_N, a query kind other than the two, an any-hit record under NART_TRACE_PACKET.  n == 0: NART_OK, nothing launched.  Multi-device contexts run it on their first device. */
#define NART_TRACE_IN_WORDS 8
#define NART_TRACE_OUT_WORDS 32
#define NART_TRACE_NO_HIT 0xFFFFFFFFu
enum { NART_TRACE_CLOSEST = 0, NART_TRACE_ANY = 1 };
enum {
    NART_TRACE_PLAIN = 0, NART_TRACE_LDS = 1, NART_TRACE_STEP = 2, NART_TRACE_STEP_ROT = 3, NART_TRACE_PACKET = 4,
    NART_TRACE_N_VARIANTS = 5
};
int nart_hip_trace(nart_ctx* ctx, uint32_t variant, uint32_t sk, int count, const float* in, uint32_t n,
                   uint32_t* out);

/* Device scene probe (test hook, never launched by a render): one scene-bound device function of the
   render path (patterns, lights, BSDF set-up, medium) on n caller-supplied records against the context's
   own device scene, one lane per record, 256-lane blocks.  in: n records of NART_SCENE_IN_WORDS (16)
   floats; out: n records of NART_SCENE_OUT_WORDS (32) floats; integer fields (u32) travel as their
   bits; input words an op does not name are ignored and output words it does not name are 0.

     op               in                                            out
     TEX_FETCH        0 u32 texture, 1 su, 2 sv, 3 u32 rough        0-2 rgb (tex_fetch)
     ENV_PDF          0 u32 light (an environment light), 1-2 st    0 env_ptn_pdf
     LIGHT_LI         0 u32 light, 1-3 p, 4-6 wi (as given),        0-2 Li, 3 pdf, 4 tMax
                      7 u32 want pdf (0: a null pdf pointer),
                      8 theta_in (NaN: formed in the function),
                      9 preset pdf, 10 preset tMax
     LIGHT_BOUND      as LIGHT_LI (7-9 ignored)                     4 tMax (light_bound)
     LIGHT_SAMPLE_LI  0 u32 light, 1-3 p, 4-5 sample,               0-2 Li, 3 pdf, 4 tMax, 5-7 wi
                      9 preset pdf, 10 preset tMax
     CREATE_BSDF      0 u32 material, 1-2 st, 3-5 sn, 6-8 dpds,     0-2 n, 3-5 n_t, 6-8 n_b, 9 u32 num,
                      9 alphaTweak                                  10-20 b[0], 21-31 b[1]: u32 type, u32 flags,
                                                                    rho (3), tau (3), eta, alpha_0, alpha_prime
                                                                    (a lobe the BSDF does not have is all 0)
     DG_LOOKUP        0-2 p (grid coordinates)                      0 dg_lookup on the global grid, 1 on the LDS copy
                                                                    k_render_volume_sm stages (grids above its
                                                                    4,096 cells: the global grid again), 2 dg_lookup2
                                                                    (2x2x2 grids, else 0), 3 u32 1 where 2 is set
     MEDIUM_WALK      0-2 o, 3-5 d (as given)                       0 u32 medium_sample_ray's answer, 1 u32 segments
                                                                    listed, 2 tCurrent and 3 tMax after it, then per
                                                                    maj_next call that returns true, up to
                                                                    NART_SCENE_WALK_SEGMENTS (7): sigma, t0, t1,
                                                                    u32 majorant index used (4 words from word 4)

   A preset is what the output variable holds before the call: light_li leaves pdf and tMax alone on a
   miss, light_sample_li's environment branch leaves pdf alone on a row of zero texels.

   build: the (ENV, FM) pair of the path kernels that the light and BSDF ops are compiled for, exactly the
   builds the renderer has: NART_SCENE_BUILD_ENV_ALL (true, NART_FT_ALL), _ALL (false, NART_FT_ALL),
   _DIFFUSE (false, Lambert + disk), _GLASS (false, Lambert + glass + disk), _ENVTEX (true, Lambert +
   plastic + environment + textures + normal maps).  The scene must fit the build by the renderer's rule:
   its feature mask (nart_hip_scene_features) inside the build's mask, no environment light under an ENV =
   false build, one under _ENVTEX.  The other ops ignore the build, which must still fit.

   NART_E_INVALID: a null pointer, an unknown op or build, n above NART_EVAL_MAX_N (all before the
   context is touched); a build the scene does not fit; DG_LOOKUP or MEDIUM_WALK on a scene without a
   medium; a record whose texture, light or material index is outside the scene; an ENV_PDF record whose
   light is no environment light or whose coordinates index outside the light's distribution, a LIGHT_SAMPLE_LI record for a textured
   environment light whose sample is outside [0, 1] (both checked on the host: nothing is launched).
   n == 0: NART_OK, nothing launched.  Multi-device contexts run it on their first device. */
#define NART_SCENE_IN_WORDS 16
#define NART_SCENE_OUT_WORDS 32
#define NART_SCENE_WALK_SEGMENTS 7
enum {
    NART_SCENE_TEX_FETCH = 0, NART_SCENE_ENV_PDF = 1, NART_SCENE_LIGHT_LI = 2, NART_SCENE_LIGHT_BOUND = 3,
    NART_SCENE_LIGHT_SAMPLE_LI = 4, NART_SCENE_CREATE_BSDF = 5, NART_SCENE_DG_LOOKUP = 6, NART_SCENE_MEDIUM_WALK = 7,
    NART_SCENE_N_OPS = 8
};
enum {
    NART_SCENE_BUILD_ENV_ALL = 0, NART_SCENE_BUILD_ALL = 1, NART_SCENE_BUILD_DIFFUSE = 2, NART_SCENE_BUILD_GLASS = 3,
    NART_SCENE_BUILD_ENVTEX = 4, NART_SCENE_N_BUILDS = 5
};
int nart_hip_scene_eval(nart_ctx* ctx, uint32_t op, uint32_t build, const float* in, uint32_t n, float* out);

/* Splat filter-index thresholds (host only, no device): thr65[k] = the least d2 whose AddSample
   filter index (render.cpp:43-49) is >= k.  NART_E_INVALID when filter_width is too small for
   them (the splat then evaluates sqrt and division per pair). */
int nart_hip_splat_thresholds(float filter_width, float* thr65);

/* Splat filter weight by d2 cell (host only): cell c holds the floats whose bits >> 16 equal
   b0 + c, as {threshold t, weight below t, weight at or above t, 0} (at most one threshold per
   cell), cells4 with room for 2048 cells.  NART_E_INVALID where the thresholds do not apply. */
int nart_hip_splat_lut(float filter_width, float* cells4, uint32_t* n_cells, uint32_t* b0);

/* Environment-map CDF search (host only, no device; test hook for the guide tables of
   path.h guided_search): for each of values[0, m), the reference's BinarySearch over v[0, n)
   (util.cpp:4-20) into full[] and the guided search into guided[].  Returns 1 if a guide table
   was built for v (non-decreasing, NaN-free, n < 2^16), 0 if not (the guided search is then the
   full search), NART_E_INVALID on bad arguments. */
int nart_hip_env_search(const float* v, uint32_t n, const float* values, uint32_t m, uint32_t* full,
                        uint32_t* guided);

/* Acceleration structure the context would build for a scene (host only, no device): BVH2 node
   count, traversal stack depth (levels; the device keeps 8 B per level per lane in LDS) and the
   triangles in leaves.  Deep trees are capped (median splits past 40 levels), so stack_depth
   stays <= 72; nart_hip_create returns NART_E_UNSUPPORTED if the stack would not fit in LDS. */
typedef struct nart_bvh_info {
    uint32_t num_nodes;
    uint32_t stack_depth;
    uint32_t num_leaf_tris;
    uint32_t reserved;
} nart_bvh_info;
int nart_hip_bvh_info(const nart_scene_blob* scene, nart_bvh_info* out);

/* Test hooks (read only): the acceleration structure itself, copied to the host.
       nodes      num_nodes BVHNode records of 64 B (device/dscene.h: lo0[3] hi0[3] lo1[3] hi1[3]
                  child[2] pad[2]; child >= 0 an inner node, < 0 a leaf ~(first << 5 | (count - 1)))
       tri_isect  num_leaf_tris triangle test records of 16 floats, leaf order
       tri_perm   3 * num_leaf_tris permuted records of 16 floats (axis-major; the trailing padding
                  records of the device buffer are not copied)
   and in info the counts, root_code (the traversal's root: 0, or a leaf code when the tree is one
   leaf, -1 when it is empty), pad (what every child box was grown by) and stack_depth.
   Capacities are in nodes (nodes_cap) and floats (isect_cap, perm_cap).  info is always filled; with
   all three buffers null the call is a size query.  NART_E_INVALID: a null ctx / scene or info, only
   some buffers null, or a capacity that is too small (nothing is copied then).
   nart_hip_bvh_dump (host only, no device): the binned-SAH tree nart_hip_create builds by default,
   with the padding and the octree words it would have there.
   nart_hip_context_bvh_dump: the tree the context built, host SAH or device LBVH (on_device = 1).
   A multi-device context dumps its first device's tree (every device builds its own from the same
   scene). */
typedef struct nart_bvh_dump_info {
    uint32_t num_nodes;
    uint32_t num_leaf_tris;
    uint32_t stack_depth;
    int32_t root_code;
    float pad;
    uint32_t on_device;
} nart_bvh_dump_info;
int nart_hip_bvh_dump(const nart_scene_blob* scene, nart_bvh_dump_info* info, void* nodes, size_t nodes_cap,
                      float* tri_isect, size_t isect_cap, float* tri_perm, size_t perm_cap);
int nart_hip_context_bvh_dump(const nart_ctx* ctx, nart_bvh_dump_info* info, void* nodes, size_t nodes_cap,
                              float* tri_isect, size_t isect_cap, float* tri_perm, size_t perm_cap);

/* The acceleration structure a context built: nodes, stack depth, leaf triangles; reserved = 1
   when it was built on the device (NART_BVH_BUILD=device: a linear BVH, device/lbvh.h; default
   the host's binned SAH), and the build time in ms (host wall clock, uploads included). */
int nart_hip_context_bvh(const nart_ctx* ctx, nart_bvh_info* out, double* build_ms);

/* Kernel variant (all render bit-identical images):
   0 = megakernel with a wave ray queue (default; scenes whose BVH is too deep for its 512-lane
       LDS layout run variant 3's kernel),
   3 = megakernel, one lane per pixel, each query traced to completion.
   1 (the wavefront variant, 2x slower) and 2 (variant 3 with a traversal quorum) were retired:
   NART_E_UNSUPPORTED. */
int nart_hip_set_variant(nart_ctx* ctx, int variant);

/* Scene-specialised path kernels (no reference counterpart; all builds render the same image).
   The context derives a feature mask from the scene (material kinds, light kinds, textured
   patterns, normal maps: NART_FT_* bits, device/path.h FT_*) and runs the ray-queue kernel built
   for the first mask that covers it -- glassSphere's, the Cornell box's, C4's -- so that code for
   kinds the scene lacks is not compiled into the kernel; throughput-bound launches (whole frames)
   of scenes whose traversal stack fits take the lean build of that mask (no priority lanes or
   speculative pairs, three waves per SIMD: NART_SCHED_LEAN).  mode 0 forces the generic build, 1
   the specialised builds without the lean one, 2 (default) all of them.  nart_hip_scene_features
   reports the scene's mask and the mask of the build the last render launched (0x3FF = generic). */
int nart_hip_set_specialize(nart_ctx* ctx, int mode);
int nart_hip_scene_features(const nart_ctx* ctx, uint32_t* features, uint32_t* build);
/* Host only (no device): the feature mask a context would derive for a scene. */
int nart_hip_scene_features_of(const nart_scene_blob* scene, uint32_t* features);
#define NART_FT_LAMBERT 0x1u
#define NART_FT_SPECULAR 0x2u
#define NART_FT_GLASS 0x4u
#define NART_FT_GLOSSY 0x8u
#define NART_FT_PLASTIC 0x10u
#define NART_FT_DISK 0x20u
#define NART_FT_RING 0x40u
#define NART_FT_ENVIRONMENT 0x80u
#define NART_FT_TEXTURE 0x100u
#define NART_FT_NORMAL_MAP 0x200u
#define NART_FT_ALL 0x3FFu

/* Splat kernel (all bit-identical): -1 = automatic (the default: 4 when the launch fills >= 1
   wave per SIMD, else 5), 4 = skewed-time tile columns over the pixel-major sample layout (each
   sample fetched once per bucket), 5 = the same with one lane per (tile column, row class), for
   small launches, 3 = four tile pixels per lane over the sample-major layout;
   1, 0 = one tile pixel per lane with the threshold / direct filter-index arithmetic (2 = 1).
   Modes fall back to a lower one where their preconditions (power-of-two buckets <= 32, filter
   bounds 1-3, threshold table and weight LUT) do not hold.  (An LDS-staged mode, an unskewed
   tile-column sweep and a compare-only one-pixel mode measured slower and were retired.) */
int nart_hip_set_splat_mode(nart_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif
