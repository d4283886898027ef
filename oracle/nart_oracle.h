/*
 * nart_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of shanesimmsart/nart's render path (RenderSession::Render and everything
 * below it), written in plain C from the reference sources.  It is the checker for the HIP
 * path and the timed CPU baseline ("kind": "port").  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it; the product never links or calls it.
 *
 * PARITY UNPINNED: the reference ships no tests, golden vectors or fixture images, and it
 * cannot be built in this image (it needs GLM, OpenEXR/Imath, oneTBB and nlohmann 3.11 via
 * CMake FetchContent; building it against stand-in headers is not allowed).  The restatement
 * is pinned only where a third-party dependency's arithmetic can be checked here: glibc 2.35
 * sinf/cosf (used through glm::sin/cos) are called directly, and the device port of them is
 * checked exhaustively against this libm (tests/test_libm_parity.py).  GLM 0.9.9.8 operation
 * order is restated from its published scalar code paths (DESIGN.md lists the assumptions).
 */
#ifndef NART_ORACLE_H
#define NART_ORACLE_H

#include "../include/nart_scene.h"
#include "../include/nart_hip.h" /* declarations only: the NART_EVAL_* ops and record layout of oracle_eval */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oracle_scene oracle_scene;

/* Builds the reference octree BVH (bvh.cpp:252-326) and light/material views of the blob.
   The blob must stay alive while the oracle scene is used. */
int oracle_create(const nart_scene_blob* blob, oracle_scene** out);
void oracle_destroy(oracle_scene* s);

/* RenderSession::Render (render.cpp:114-206) with `threads` workers on a dynamic bucket
   queue (tbb::task_group stand-in).  image: totalW*totalH Pixels. */
int oracle_render(oracle_scene* s, const nart_render_params* p, nart_pixel* image, int threads);

/* Path counts of one render, summed over the worker threads (each worker counts privately and adds
   its totals once, so concurrent renders do not mix and counting changes no rendered bit):
     EXTENSION   closest-hit queries of Li_alpha: the camera ray plus one per continued bounce
                 (pathintegrator.cpp:184)
     SHADED      those queries that found a surface -- every hit the integrator goes on to process,
                 the lower-priority interfaces it only steps through included
     VISIBILITY  occlusion queries of EstimateDirect (pathintegrator.cpp:72 and :105)
     SAMPLES     camera samples traced (extra rows and columns included) */
enum { ORACLE_N_EXTENSION = 0, ORACLE_N_SHADED = 1, ORACLE_N_VISIBILITY = 2, ORACLE_N_SAMPLES = 3, ORACLE_N_COUNTS = 4 };

/* oracle_render that also reports the render's path counts: counts[ORACLE_N_COUNTS] (or NULL). */
int oracle_render_counted(oracle_scene* s, const nart_render_params* p, nart_pixel* image, int threads,
                          uint64_t* counts);

/* RenderTile for a list of bucket ids into tiles[i] (tile_size^2 Pixels each). */
int oracle_render_buckets(oracle_scene* s, const nart_render_params* p, const uint32_t* ids,
                          uint32_t n, nart_pixel* tiles, int threads);

/* Per-sample Li_alpha for pixels [x0,x0+w) x [y0,y0+h): out[((y-y0)*w+(x-x0))*spp+i][4];
   uv (optional) receives the Latin-square image samples [..][2]. */
int oracle_render_samples(oracle_scene* s, const nart_render_params* p, uint32_t x0, uint32_t y0,
                          uint32_t w, uint32_t h, float* out, float* uv);

/* Stats of the reference octree build (for tests of Q14 and the chunk-index quirk).
   grid_res[0..2] = grid resolution, grid_res[3] = triangles reachable by traversal. */
int oracle_bvh_stats(const oracle_scene* s, uint32_t* n_chunks, uint32_t* max_chunk_tris,
                     uint32_t* root_is_leaf, uint32_t* grid_res);

/* Individual primitives for known-answer tests. */
void oracle_rng_stream(uint32_t seed, uint32_t n, float* out);
void oracle_latin_square(uint32_t seed, uint32_t spp, float* out_xy, uint32_t* rng_state_after);
float oracle_fresnel(float eta_o, float eta_i, float cos_theta);
/* BinarySearch (util.cpp:4-20) as the environment light's CDF inversion uses it. */
uint32_t oracle_binary_search(float value, const float* v, uint32_t start, uint32_t end);
/* One function of the restatement (fresnel, bxdf_f / bxdf_pdf / bxdf_sample_f, sample_wh, the
   sampling functions, the rng, f2u32 / f2u8, gmod / gfract) or of the linked libm (acosf, atanf,
   atan2f, logf, sinf / cosf) on n caller-supplied inputs.  op and the 16-float records in and out are
   those of the device probe nart_hip_eval (NART_EVAL_*, include/nart_hip.h), of which this is the
   CPU side; BXDF_F_PDF answers (bxdf_f, bxdf_pdf), LOGF_LDS answers logf.  0, or -1 for an unknown
   op or a null pointer. */
int oracle_eval(uint32_t op, const float* in, uint32_t n, float* out);
/* oracle_trace over n rays: the CPU side of the device probe nart_hip_trace, whose records these are
   (include/nart_hip.h: NART_TRACE_IN_WORDS words in -- origin, tMax, direction, query kind -- and
   NART_TRACE_OUT_WORDS words out per ray).  Out: 0 the triangle the reference octree returns or
   0xFFFFFFFF (any-hit: 1 when the search with tMax preset finds a hit, else 0), 1 the bits of its t
   (the preset tMax on a miss; any-hit: 0), 2 the ORACLE_TRACE_* class flags, 3-4 the strictly closest
   triangle over all triangles and the bits of its t (brute force; lowest index on a tie), 6-25 the
   isect_t fields of a closest hit in the probe's order (zero on a miss and for any-hit).
   0, or -1 for a null pointer. */
#define ORACLE_TRACE_NAN 1u           /* some triangle's plane distance is NaN (0/0) */
#define ORACLE_TRACE_TIE 2u           /* two triangles the ray hits (each tested alone) have bit-equal t */
#define ORACLE_TRACE_NOT_BRUTE 4u     /* the octree's answer is not the brute-force closest hit */
#define ORACLE_TRACE_TIE_CLOSEST 8u   /* ... and that t is the closest one */
#define ORACLE_TRACE_NAN_ACCEPTED 16u /* a NaN-plane triangle passes Triangle::Intersect (edge test included) */
#define ORACLE_TRACE_NAN_OUTSIDE 32u  /* ... and the ray's origin lies outside that triangle's bounds */
#define ORACLE_TRACE_GHOST 64u        /* a triangle passes with a t before the ray enters its bounds (grown by 2^-12 of the
                                         coordinates involved), or on a ray that misses them: the ray lies in its plane and
                                         t is a quotient of two roundings */
#define ORACLE_TRACE_GHOST_WINS 128u  /* the search's own answer (with or without the NaN triangles) is such a hit */
#define ORACLE_TRACE_NAN_DECIDES 256u /* the same search with NaN plane distances rejected answers differently: a NaN
                                         triangle shares the winner's chunk */
#define ORACLE_TRACE_NAN_HIDES 512u   /* ... it finds a hit where the reference's search finds none */
int oracle_trace_n(const oracle_scene* s, const float* in, uint32_t n, uint32_t* out);
/* One scene-bound function of the restatement (tex_fetch, ptn_pdf, light_li, light_sample_li, create_bsdf,
   dg_lookup, medium_sample_ray + the majorant iterator) on n caller-supplied records against s: the CPU
   side of the device probe nart_hip_scene_eval, whose ops (NART_SCENE_*) and records -- 16 floats in, 32
   out -- these are (include/nart_hip.h).  LIGHT_BOUND answers light_li's tMax; the three DG_LOOKUP words
   are dg_lookup; theta_in is ignored (the restatement always forms it).  The reference indexes its tables
   without checks and some inputs run off them on x86 (a NaN texture coordinate: (int)NaN is INT_MIN), so
   every table read made here -- texel, mpdf / cpdf / mcdf / ccdf, density corner -- is bounds-checked:
   on a miss the read is not made and flags[i] is ORACLE_SCENE_OOB (such a record must never be sent to
   the device); else flags[i] is 0.  (The majorant index is checked by the restatement itself.)
   0, or -1: a null pointer, an unknown op, a medium op without a medium, a texture / light / material
   index outside the scene, ENV_PDF on a light that is no environment light. */
#define ORACLE_SCENE_OOB 1u
int oracle_scene_eval(const oracle_scene* s, uint32_t op, const float* in, uint32_t n, float* out, uint32_t* flags);
/* Test statistic: the longest nested-dielectric list a path of this process reached (reset: zero it). */
uint32_t oracle_max_list(int reset);

#ifdef __cplusplus
}
#endif
#endif
