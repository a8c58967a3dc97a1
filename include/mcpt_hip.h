/*
 * mcpt_hip.h — C ABI of the MI355X path-tracing hot path (libmcpt_hip.so).
 *
 * The reference drives its per-sample loop through C++ module interfaces
 * (MonteCarloPathTracing/ is abbreviated MCPT/ below):
 *   RayGeneration::init/generateRay        MCPT/raygeneration.h:15-17, raygeneration.cpp:29-67
 *   SceneBuild::buildScene/init            MCPT/scenebuild.h:31-33,   scenebuild.cpp:50-101,149-169
 *   SceneBase::intersect/shade             MCPT/scenebuild.h:15-16,   scenebuild.cpp:103-145
 *   ColorOut::init/outputColorCL           MCPT/colorout.h:6-8,       colorout.cpp:31-73
 *   OpenCL::init/update (the frame loop)   MCPT/OpenCLApp.h:4-5,      OpenCLApp.cpp:36-82
 *   ThirdPartyWrapper::loadObject/outputPicture  MCPT/thirdpartywrapper.h:13-16
 *   Auxiliary::parseCamera                 MCPT/auxiliary.h:27,       auxiliary.cpp:20-71
 *   BVH::HLBVH<CPU>                        MCPT/BVH/hlbvh.h:10-26,    hlbvh.cpp:92-200
 * Every entry point below names the interface it replaces.
 *
 * Conventions
 *  - Plain C: POD structs, pointers + sizes, int status (0 = MCPT_OK, < 0 =
 *    error), no exceptions cross the boundary; mcpt_last_error() explains the
 *    last failure of the calling thread.
 *  - Record structs are byte-identical to MCPT/objdef.h:21-99 (Camera 80 B,
 *    Ray 48 B, Hit 48 B, Triangle 64 B, Material 48 B, BVHNode 64 B), so a
 *    reference host can hand its own vectors over unchanged.
 *  - "_dev" pointers are device (HBM) pointers, "stream" is a hipStream_t
 *    passed as void* (NULL = default stream).  Host pointers are never
 *    retained after a call returns.
 *  - A context is bound to one GPU and is not thread-safe: one host thread or
 *    process per GPU (multi-GPU = one process per GPU).
 */
#ifndef MCPT_HIP_H
#define MCPT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- status */
#define MCPT_OK 0
#define MCPT_ERR_ARG (-1)      /* bad argument / size mismatch              */
#define MCPT_ERR_HIP (-2)      /* HIP runtime failure                        */
#define MCPT_ERR_IO (-3)       /* file could not be read / written           */
#define MCPT_ERR_PARSE (-4)    /* malformed OBJ / MTL / JSON                 */
#define MCPT_ERR_LIMIT (-5)    /* BVH deeper than the reference's stack[64]  */
#define MCPT_ERR_NOGPU (-6)    /* no HIP device / device index out of range  */

/* ------------------------------------------------------ records (objdef.h) */
typedef struct mcpt_camera {        /* objdef.h:21-27, 80 B */
  float center[4], direction[4], up[4], horizontal[4];
  float arg;                        /* vertical fov in radians              */
  float tmin;
  uint32_t camera_type;             /* 0 perspective, 1 orthographic        */
  float pad;
} mcpt_camera;

typedef struct mcpt_ray {           /* objdef.h:29-39, 48 B */
  float origin[4];                  /* .w bits: int term_depth              */
  float direction[4];               /* .w bits: int pixel id                */
  float ratio[4];                   /* unused by the reference              */
} mcpt_ray;

typedef struct mcpt_hit {           /* objdef.h:41-48, 48 B */
  float normal[4];
  float point[4];
  float t;                          /* FLT_MAX = miss                       */
  uint32_t triangle_id;
  uint32_t material_id;
  uint32_t pad;
} mcpt_hit;

typedef struct mcpt_triangle {      /* objdef.h:50-56, 64 B */
  float v[3][4];
  float normal[4];                  /* .w bits: int material id             */
} mcpt_triangle;

enum {                              /* objdef.h:58-67 */
  MCPT_DIFFUSE = 1,
  MCPT_GLOSSY = 2,
  MCPT_TRANSPARENT = 3,
  MCPT_LIGHT = 4
};

typedef struct mcpt_material {      /* objdef.h:69-79, 48 B */
  int32_t type;
  float Ni, Ns, pad;
  float kd[4];
  float ka_ks[4];                   /* ka for LIGHT, ks for GLOSSY          */
} mcpt_material;

typedef struct mcpt_bvh_node {      /* objdef.h:91-99, 64 B */
  float bbmin[4], bbmax[4], pad[4];
  int32_t parent, left, right, pad2;/* leaf: left == right == triangle id   */
} mcpt_bvh_node;

/* ray.origin.w / term_depth bitfield (shade.cl:100-206) */
#define MCPT_TERMINATED 0xFF000000u
#define MCPT_INSIDE     0x00FF0000u
#define MCPT_DEPTH_MASK 0x0000FFFFu

/* -------------------------------------------------------- opaque handles */
typedef struct mcpt_ctx mcpt_ctx;
typedef struct mcpt_scene mcpt_scene;

/* Render modes for the fused path.
 *  MCPT_MODE_EXACT   — reference arithmetic, traversal order and tie rule;
 *                      closest-hit pruning only where it cannot change the
 *                      accepted hit.  The default.
 *  MCPT_MODE_NOPRUNE — exhaustive left-first traversal exactly as
 *                      objdef.h:240-275 (slow; parity cross-check).          */
#define MCPT_MODE_EXACT   0
#define MCPT_MODE_NOPRUNE 1

typedef struct mcpt_render_params {
  int32_t width, height;            /* config width/height (= camera.resolution) */
  int32_t max_depth;                /* config "maxdepth"  (-D MAX_DEPTH)   */
  int32_t max_attempt;              /* config "attempt"   (-D MAX_ATTEMPT) */
  int32_t frame_begin;              /* first frame index of this call (attemptCount) */
  int32_t frames;                   /* frames to render in this call       */
  int32_t stripe_rows;              /* multi-GPU tile: rows per stripe      */
  int32_t stripe_index;             /* this GPU's stripe residue            */
  int32_t stripe_count;             /* number of GPUs (1 = whole image)     */
  int32_t mode;                     /* MCPT_MODE_*                          */
  int32_t frames_per_launch;        /* frames per block (a lane runs one pixel
                                       for one block, then hands it on);
                                       <= 0: auto (mcpt_tuning.block_entries);
                                       images over 67 M pixels (no hand-off
                                       area) run one block of at most
                                       max_block_frames frames per launch */
  int32_t schedule;                 /* MCPT_SCHED_*: how k_render batches leaf
                                       tests (results identical; speed only) */
  int32_t jitter;                   /* 0 (a zero-initialised struct): every frame
                                       shoots the reference's ray through the
                                       pixel's corner; 1: sub-pixel jitter
                                       (antialiasing, see mcpt_render_frames);
                                       any other value is MCPT_ERR_ARG        */
} mcpt_render_params;

/* Leaf-test schedules of the fused kernel (bit-identical results):
 *  MCPT_SCHED_SINGLE — one triangle per lane per leaf phase (the value of a
 *                      zero-initialised mcpt_render_params)
 *  MCPT_SCHED_PAIRED — a lane whose next stack entry is also a leaf tests
 *                      both in one phase (measured faster on C2-C5: +2-9 %;
 *                      the Python host's default);
 *  Renderer.tune_schedule() picks one by timing both. */
#define MCPT_SCHED_SINGLE 0
#define MCPT_SCHED_PAIRED 1

typedef struct mcpt_stats {
  uint64_t segments;                /* rays alive at intersect entry, all frames */
  uint64_t node_visits;             /* nodes whose children were tested (EXACT: 4-wide) */
  uint64_t tri_tests;               /* triangle tests                        */
  uint64_t bad_material;            /* hits on an unknown material type      */
  double   kernel_ms;               /* device time of the last render call   */
  int32_t  launches;                /* kernel launches of the last render call */
  int32_t  frames_per_block;        /* block size the last render call used   */
  uint64_t wave_node_phases;        /* wave-level node steps (SIMT efficiency = */
  uint64_t wave_leaf_phases;        /*  node_visits / (64 * wave_node_phases)) */
  uint64_t wave_shade_phases;
  uint64_t order_fallbacks;         /* EXACT: segments re-searched in the     */
                                    /*  reference's left-first order         */
  uint64_t wave_iterations;         /* k_render loop iterations, all waves    */
  uint64_t lane_waiting;            /* lane-iterations spent waiting for the
                                       previous frame block of its pixel     */
  uint64_t lane_idle;               /* lane-iterations with no pixel (queue
                                       claim pending, or the launch's tail)  */
  int32_t  stack_window;            /* 1: the last call ran the LDS-window stack */
  int32_t  workgroups;              /* 64-lane waves per launch (the resident grid;
                                       a k_render workgroup holds 4 of them)      */
  uint64_t debug_violations;        /* MCPT_DEBUG builds: stack-bound, node- and
                                       triangle-index violations k_render caught
                                       (always 0 in release builds)           */
  uint64_t phase_ticks[4];          /* MCPT_PHASE_TIMING builds: shader-clock ticks
                                       all waves spent in fetch, T, L, S (0 in
                                       release builds)                        */
  uint64_t leaf_rejects;            /* stats on, quantized tree: leaves the search
                                       reached whose exact box the ray misses */
  int32_t  quantized;               /* 1: the last call searched the 64-B
                                       quantized tree (EXACT mode)            */
  int32_t  primary_cache;           /* 0: the last call traced every frame's
                                       primary ray; 1: it read the cached
                                       primary hits; 2: it computed them too
                                       (always 0 for a jittered call)         */
  double   primary_ms;              /* primary_cache 2: device time of the
                                       primary-hit pass (part of kernel_ms)   */
  int32_t  top_levels;              /* the search tree's top levels the last
                                       call kept in LDS (mcpt_tuning.top_levels) */
} mcpt_stats;

/* Launch-plan knobs of the fused kernel (speed only: every setting gives the
 * same bits).  A zero-initialised struct means "defaults"; each field <= 0
 * keeps its default.  Replaces the environment knobs of earlier builds:
 * nothing is read from the environment on the render path. */
typedef struct mcpt_tuning {
  int32_t leaf_threshold;   /* lanes with a pending leaf before the L phase runs,
                               for a wave of 64 live lanes (default 4 single /
                               16 paired schedule; scaled to the live lanes)   */
  int32_t shade_threshold;  /* lanes waiting before the S phase runs, for 64
                               live lanes (32; scaled the same way)            */
  int32_t queue_chunk;      /* queue entries a wave claims per atomic (4)        */
  int32_t block_entries;    /* auto frames-per-block: smallest block count (at
                               least 2) that gives every resident lane this many
                               queue entries (8)                                 */
  int32_t max_block_frames; /* frames-per-block upper bound of auto plans and of
                               images over 67 M pixels (32)                      */
  int32_t stack_window;     /* 0 auto (default), 1 the 32-entry LDS window with
                               a global spill, 2 the whole stack in LDS          */
  int32_t lds_pad;          /* extra LDS bytes per workgroup (occupancy
                               experiments; 0)                                    */
  int32_t queues;           /* work queues (1..8; 8: one per XCD)              */
  int32_t fetch_threshold;  /* lanes of a wave needing a new queue entry before
                               the wave claims and starts them together (1)    */
  int32_t quantized;        /* EXACT search tree: 0 auto (the 64-B quantized
                               nodes when the 128-B tree exceeds 32 MiB, the
                               GPU's aggregate L2; the 96-B exact nodes for
                               trees over 1 MiB up to that; the 128-B nodes
                               below), 1 quantized whenever the
                               scene has them, 2 the 128-B nodes, 3 the 96-B
                               exact nodes whenever the scene has them (trees
                               up to 32 MiB; six gathers a node step, not
                               seven)                                            */
  int32_t primary_cache;    /* every frame re-shoots the same primary ray, so its
                               hit is computed once per (scene, camera, image,
                               stripes, mode) and kept in the context: 0 auto
                               (a call of >= 2 frames, or a one-frame call of
                               the previous call's view, computes it; every
                               call with a matching one reads it), 1 always,
                               2 never; a jittered call (mcpt_render_params
                               .jitter) neither reads nor builds it             */
  int32_t last_block_frames; /* auto frames-per-block, one-launch calls of two
                               or more blocks: the last block of every pixel
                               is this many frames and the others share the
                               rest evenly (a short last block shortens the
                               launch's tail); 0 auto (ceil(frames / 8) from
                               6 pixels per resident lane, ceil(frames / 4)
                               from 2.5 on a whole image (stripe_count 1),
                               else equal blocks), -1 equal blocks            */
  int32_t tile_order;       /* order of the 8x8 pixel tiles in the work queues:
                               0 auto (the primary-hit pass measures each
                               pixel's primary-ray traversal; tiles whose
                               costliest pixel is dearest start first, so the
                               longest per-pixel chains do not start last), 1
                               the image order, 2 by the tile's summed cost    */
  int32_t pixel_spread;     /* how the queues' pixel slots map to a wave's
                               lanes: 0 auto (spread up to 2.5 pixels per
                               resident lane: strong-scaled shares, where each
                               pixel's own chain sets the time; tile-major
                               above), 1 tile-major (a wave's 64
                               consecutive slots are one 8x8 tile), 2 spread
                               (they are one pixel of each of 64 tiles, so one
                               tile's dear pixels run in different waves)      */
  int32_t top_levels;       /* EXACT: the search tree's top levels kept in LDS,
                               where a segment descends through them as it
                               begins instead of one T-phase gather per level:
                               0 auto (2; 4 on trees over 4 MiB), 1-4 levels,
                               -1 none                                           */
} mcpt_tuning;

/* ------------------------------------------------------- version / errors */
/* The ABI revision this header describes.  It changes whenever a struct
 * passed across the boundary changes size or layout, or an entry point its
 * arguments (3: mcpt_tuning's tile_order / pixel_spread,
 * mcpt_set_pixel_segments' capacity; 4: the rejected T-phase-helper and
 * merged-gather knobs and counters removed from mcpt_tuning / mcpt_stats,
 * `top_levels` added to both; 5: `jitter` appended to mcpt_render_params,
 * mcpt_generate_rays_jittered added).  A new struct with a new entry point
 * changes neither, so mcpt_denoise_params and mcpt_denoise came in at 5, and
 * so did mcpt_environment with mcpt_scene_set_environment, mcpt_env_eval and
 * mcpt_decode_hdr, and the vertex-normal entry points (mcpt_vertex_normals,
 * mcpt_load_obj_normals, mcpt_obj_normals_from_text,
 * mcpt_scene_set_vertex_normals, mcpt_shading_normals): functions only.
 * The texture entry points (mcpt_load_obj_uvs, mcpt_obj_uvs_from_text,
 * mcpt_load_mtl_maps, mcpt_mtl_maps_from_text, mcpt_scene_set_textures with
 * its own mcpt_textures, mcpt_texture_eval) came in at 5 likewise, and so
 * did the thin lens (mcpt_render_frames_lens and mcpt_generate_rays_lens with
 * their own mcpt_lens) and the normal-map entry points
 * (mcpt_load_mtl_bump_maps, mcpt_mtl_bump_maps_from_text,
 * mcpt_scene_set_normal_maps with its own mcpt_normal_maps, mcpt_bump_eval).
 * A binding checks mcpt_abi_version() == MCPT_ABI_VERSION once at load and
 * refuses a library built from another header.                           */
#define MCPT_ABI_VERSION 5
int32_t mcpt_abi_version(void);
const char *mcpt_version(void);
const char *mcpt_last_error(void);

/* ----------------------------------------------------------- host side
 * Everything here is plain C++ on the host; no GPU needed.               */

/* Auxiliary::parseCamera (auxiliary.cpp:20-71): JSON camera -> Camera.   */
int mcpt_parse_camera(const double position[3], const double lookat[3],
                      const double up[3], double fov_deg, mcpt_camera *out);

/* MTL record -> Material, thirdpartywrapper.cpp:65-97 precedence:
 * ior != 1 -> TRANSPARENT; any Ka > 0 -> LIGHT; Ns != 1 -> GLOSSY; else DIFFUSE. */
int mcpt_classify_material(float ior, const float ambient[3], const float diffuse[3],
                           const float specular[3], float shininess, mcpt_material *out);

/* ThirdPartyWrapper::loadObject (thirdpartywrapper.cpp:25-99) on an
 * OBJ + its MTL library: two-call pattern — call with NULL outputs to get
 * the counts, then again with arrays of that size.  Triangles come out
 * with v[] filled and normal zeroed (SceneCL packs them, below);
 * mat_index[i] is the per-face material index (-1 if none).            */
int mcpt_load_obj(const char *directory, const char *objname,
                  mcpt_triangle *tris, int32_t *mat_index, int64_t *n_tris,
                  mcpt_material *mats, int32_t *n_mats);

/* SceneCL ctor packing (scenebuild.cpp:58-62): normal = normalize(cross(
 * v1-v0, v2-v0)), normal.w <- material index bits.  In place.           */
int mcpt_pack_triangles(mcpt_triangle *tris, const int32_t *mat_index, int64_t n);

/* HLBVH<CPU>::build (hlbvh.cpp:92-200): Morton LBVH, 2n-1 nodes, root 0,
 * leaves at [n-1, 2n-2].  nodes must hold 2n-1 records.                 */
int mcpt_build_hlbvh(const mcpt_triangle *tris, int64_t n, mcpt_bvh_node *nodes);

/* Max DFS stack depth the reference traversal needs on this tree.      */
int mcpt_bvh_stack_depth(const mcpt_bvh_node *nodes, int64_t n_nodes, int32_t *depth);

/* BVH::TEST::SAH (bvhtest.cpp:97-108), the "testbvh" SAH line: the float
 * result (Cinn * area of nodes [0, size/2) + Ctri * area of the rest, summed
 * in double, over the root's area) widened to double.                     */
int mcpt_bvh_sah(const mcpt_bvh_node *nodes, int64_t n_nodes, double *sah);

/* ThirdPartyWrapper::outputPicture (thirdpartywrapper.cpp:14-23):
 * stbi_write_hdr with vertical flip, 4 components in, RGB out.           */
int mcpt_write_hdr(const char *path, int32_t width, int32_t height,
                   const float *rgba, int32_t flip_vertically);
/* Same encoder into memory: returns the byte count (call with NULL first);
 * MCPT_ERR_ARG if `cap` is too small for it.                              */
int64_t mcpt_encode_hdr(int32_t width, int32_t height, const float *rgba,
                        int32_t flip_vertically, uint8_t *out, int64_t cap);
/* Radiance RGBE reader (the format mcpt_write_hdr writes; an environment map
 * for mcpt_scene_set_environment): `len` bytes of a file with the
 * "#?RADIANCE" (or "#?RGBE") magic, a FORMAT=32-bit_rle_rgbe line and the
 * "-Y h +X w" resolution line, run-length encoded or flat scanlines.  A
 * texel decodes as stb_image does, m * 2^(e - 136) per channel and 0 when
 * e == 0.  *width and *height are set once the header is read (rgb_out NULL:
 * the size query); then width * height * 3 floats go to rgb_out, rows in file
 * order (the first row of the file first), `cap` its capacity in floats
 * (MCPT_ERR_ARG when too small).  A parser of files from outside: a truncated
 * file, a run longer than its scanline, a scanline width that disagrees with
 * the header, a bad header or width * height > 2^26 is MCPT_ERR_PARSE, and no
 * input makes it read past `len` or write past the image.                  */
int mcpt_decode_hdr(const uint8_t *bytes, int64_t len, int32_t *width, int32_t *height,
                    float *rgb_out, int64_t cap);

/* ---------------------------------------------------------- device side */

/* OpenCLBasic::init (oclbasic.cpp:75-122) equivalent: bind to a GPU.     */
int mcpt_ctx_create(int32_t device, mcpt_ctx **out);
int mcpt_ctx_destroy(mcpt_ctx *ctx);
int mcpt_device_count(int32_t *count);

/* SceneBuild::buildScene (scenebuild.cpp:50-101,149-156): upload the packed
 * triangles + reference BVH + materials; converted to the device layout
 * (child-box nodes, Cramer-ready triangles — DESIGN.md §2) once here.   */
int mcpt_scene_upload(mcpt_ctx *ctx, const mcpt_triangle *tris, int64_t n_tris,
                      const mcpt_bvh_node *nodes, int64_t n_nodes,
                      const mcpt_material *mats, int32_t n_mats, mcpt_scene **out);
int mcpt_scene_destroy(mcpt_scene *scene);
/* The same with the scene already in HBM (tris_dev packed as
 * mcpt_pack_triangles leaves them, nodes_dev in the HLBVH layout, e.g. from
 * mcpt_build_hlbvh_device + mcpt_treelet_gpu_device): every device structure,
 * the EXACT path's SAH search tree included, built on the GPU, the same
 * bytes as mcpt_scene_upload's.  Synchronises `stream`.                  */
int mcpt_scene_upload_device(mcpt_ctx *ctx, const mcpt_triangle *tris_dev, int64_t n_tris,
                             const mcpt_bvh_node *nodes_dev, int64_t n_nodes, const mcpt_material *mats,
                             int32_t n_mats, void *stream, mcpt_scene **out);
/* Process-wide upload option, on by default: the search tree of the scenes
 * uploaded from here on (either path, up to 131072 triangles) is optimised by
 * `passes` rounds of subtree reinsertion and a collapse that keeps the plain
 * tree's stack need.  0 = the plain tree.  The tree only
 * sets the search's cost, never a result.  passes in [0, 16]; default 3.    */
int mcpt_set_sah_optimize(int32_t passes);
int mcpt_get_sah_optimize(int32_t *passes);
/* A scene's device arrays copied to the host (introspection).  which: 0 the
 * search tree (128-B nodes), 1 its quantized nodes, 2 the reference tree
 * 4-wide, 3 the binary child-box nodes, 4 triangles, 5 quantized-path
 * triangles, 6 int32[4] {stack_depth, stack_depth4, quantized, n_internal},
 * 7 the 96-B search-tree nodes, 8 their slot-indexed triangles, 9 the
 * reference tree 4-wide with its leaves relabelled to those (7-9: 0 bytes
 * where the scene has none).
 * *bytes = the size (host NULL: size only).                               */
int mcpt_scene_read(const mcpt_scene *scene, int32_t which, void *host, int64_t cap, int64_t *bytes);

/* Fused per-pixel path loop: for every pixel of this GPU's stripes and
 * frames [frame_begin, frame_begin+frames): generateRay -> maxdepth x
 * (intersect, shade) -> history accumulate, exactly the per-pixel effect of
 * OpenCL::update (OpenCLApp.cpp:57-82) + ColorOut (colorout.cpp:40-73).
 * seeds/hist/count are W*H device arrays (u32, float4, i32) that persist
 * across calls; pixels outside this GPU's stripes are left untouched.
 * Stream-ordered and asynchronous: the call enqueues its work on `stream`
 * and returns (mcpt_get_stats waits for it).  One stream per context at a
 * time: the context's queue heads and hand-off area are reused by every
 * call.
 * params->jitter = 1 (opt-in antialiasing, no reference counterpart): every
 * frame of a pixel starts with two draws from the pixel's own seed chain,
 * before any shading draw of that frame, jx = lcg15(seed) * 2^-15 and then jy
 * the same, and generateRay runs with px = ((float)idx + jx) / width,
 * py = ((float)idy + jy) / height, everything after unchanged: a box filter
 * over the pixel's footprint whose jx = jy = 0 corner is the reference's ray.
 * The history rule is untouched: a jittered pixel is still the reference's
 * mean over its non-zero samples.  Such a call neither reads nor builds the
 * primary-hit cache (mcpt_stats.primary_cache = 0) and leaves a held one
 * valid for later unjittered calls.
 * Where MCPT_MODE_EXACT may differ from the reference: a segment whose ray
 * has a direction component with 0 < |d| < 2^-126 (denormal, not zero) AND
 * its origin exactly on a box plane of the tree on that axis; there the
 * hoisted rcp(d) = +-inf makes the slab test 0 * inf = NaN where the
 * reference computes 0 / d = 0, and a triangle the reference accepts can be
 * missed.  Every other ray holds the reference's bits; MCPT_MODE_NOPRUNE
 * holds them on all rays (both measured on k_render and the primary-hit
 * pass: tests/test_gpu_intersect_edges.py, test_render_denormal_directions).  generateRay and shade.cl normalize every
 * direction, so such a component needs a camera `direction` (or a bounce)
 * with a component below 2^-126 of the largest one.  mcpt_intersect has no
 * such exception (it tests each ray and searches these literally).        */
int mcpt_render_frames(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_camera *cam,
                       const mcpt_render_params *params, uint32_t *seeds_dev,
                       float *hist_dev, int32_t *count_dev, void *stream);

/* Thin-lens camera (opt-in depth of field, no reference counterpart; ABI 5: a
 * new struct with new entry points).  radius R >= 0 and focus_distance F > 0
 * in scene units, both finite; F is measured along the view axis.
 *
 * mcpt_render_frames_lens is mcpt_render_frames with a lens.  A null lens or
 * R == 0 means no lens: no draw is taken and the call is mcpt_render_frames'
 * bit for bit, jittered or not.  R > 0 needs params->jitter == 1 (a lens needs
 * a fresh primary ray per frame), else MCPT_ERR_ARG.  R < 0, F <= 0, or either
 * not finite: MCPT_ERR_ARG, and nothing is touched.
 *
 * Draws, per pixel and frame, from the pixel's own seed chain: jx, jy as a
 * jittered frame takes them, then r1 = lcg15(seed), r2 = lcg15(seed), then the
 * frame's shading draws as before.
 * Lens sample (the helpers of randomDirection): rho = sqrt(r1 * 2^-15) with
 * the hardware square root, phi = 2 * pi * r2 / 32768 formed in double and
 * rounded to float, (s, c) = sin, cos of phi, (a, b) = (rho * c, rho * s):
 * uniform over the unit disk.
 * Ray.  (o, d): the jittered generateRay's ray for (idx + jx, idy + jy), of
 * either camera_type (the orthographic camera's o is its image-plane point, d
 * the view direction).  c^, h^, u^: normalize() of the xyz of camera.direction,
 * .horizontal and .up (horizontal and up are not unit vectors in general),
 * computed once per launch.  Then
 *     k  = F / dot(d, c^)
 *     P  = o + k * d                   the sample's point on the focus plane
 *     o' = o + R * (a * h^ + b * u^)   the point on the lens
 *     d' = normalize(P - o')
 * and o'.w, d'.w carry the bits they carried: depth 0 and the pixel id.
 * Operation order (one device function, lens_ray of mcpt_lens.h, runs in both
 * the fused kernel and mcpt_generate_rays_lens): A = R * (rho * c),
 * B = R * (rho * s), off = fma(A, h^, B * u^) per component, k by the 2.5-ulp
 * division, o' = o + off, d' = normalize(fma(k, d, -off)) (P - o' without the
 * cancelling o).
 * All lens rays of one sample meet at P, so geometry on the plane
 * dot(x - o, c^) = F images as the jitter-only render does and everything
 * else is blurred over a disk that grows linearly with its distance from that
 * plane.  Such a call is a jittered call: it neither reads nor builds the
 * primary-hit cache and leaves a held one valid.                            */
typedef struct mcpt_lens {
  float radius, focus_distance;
  float pad[2];
} mcpt_lens;
int mcpt_render_frames_lens(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_camera *cam, const mcpt_lens *lens,
                            const mcpt_render_params *params, uint32_t *seeds_dev, float *hist_dev,
                            int32_t *count_dev, void *stream);

/* The estimator (opt-in, no reference counterpart; ABI 5: a new struct with
 * new entry points).  The reference's image is not the path
 * integral: history.cl drops every all-zero sample, so a pixel holds the mean
 * over its NON-ZERO samples, and shade.cl's depth cap returns black for every
 * longer path.  An estimator changes both rules; a null estimator, or {0, 0},
 * is mcpt_render_frames_lens' call bit for bit.
 *
 * count_all = 1 (counted history): an all-zero sample is no longer skipped.
 * It runs the expression of every other sample, hist = (now + hist * cnt) /
 * (float)(cnt + 1) with the 2.5-ulp division, hist.w = 0, ++cnt; with now = 0
 * that scales the mean by cnt / (cnt + 1).  The cnt >= max_attempt stop and the
 * frame-index gate frame_begin + f <= max_attempt are unchanged, so count
 * after n frames from zero is min(n, max_attempt) for every pixel of the
 * stripes: misses, capped paths, unknown materials and black environment
 * samples included.  The flag draws no random number: without roulette the
 * seeds come out as the default render's.
 *
 * rr_depth >= 1 (Russian roulette; 0: off).  In shade, after the depth-cap
 * test, where all of these hold: the shaded material is MCPT_DIFFUSE or
 * MCPT_GLOSSY; a new ray was produced (not a rejected lobe sample that is drawn
 * again, not a cut hit, not a light, not an unknown material); the cap did not
 * end the path; the new depth (term_depth & 0xFFFF, & 0xFF on a scene with
 * cutouts: the value the cap compares) is >= rr_depth.  Then, with R the
 * reflectance this bounce multiplied into the colour (kd times the texture
 * factor on the diffuse lobe, ks where the Phong lobe was taken),
 *     p = fmin(1.0f, fmax(R.x, fmax(R.y, R.z)))
 *     u = lcg15(seed) * 2^-15          one draw, always taken
 *     u < p:  colour = colour / p      (the 2.5-ulp division, all four lanes)
 *     else:   colour = 0, term_depth |= MCPT_TERMINATED, as the cap does it.
 * p = 0 always ends the path and p = 1 never does; transparent hits and total
 * internal reflection draw nothing.  A survivor's colour is at most what R = 1
 * would have given it, so the rule makes no fireflies.  The survival
 * probability is the bounce's albedo, not the path's throughput: the
 * reference scales every bounce by 1 / 2 pi, which would make a throughput
 * rule end nearly every path.  A path the roulette ends is a zero sample that
 * must be counted, so rr_depth > 0 needs count_all = 1.
 *
 * MCPT_ERR_ARG, and nothing is touched: rr_depth > 0 with count_all = 0,
 * rr_depth < 0 or > 65535, count_all not 0 or 1 (and what
 * mcpt_render_frames_lens refuses).  pad is ignored.  One device function per
 * rule runs in the fused kernel and in the wavefront kernels below
 * (mcpt_shade_est, mcpt_accumulate_all).  The primary-hit cache is used as
 * before: it holds hits, and shading them draws as a traced hit's does.     */
typedef struct mcpt_estimator {
  int32_t count_all; /* 0 | 1 */
  int32_t rr_depth;  /* 0: off, else 1..65535 */
  int32_t pad[2];
} mcpt_estimator;
int mcpt_render_frames_est(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_camera *cam,
                           const mcpt_lens *lens /* may be NULL */, const mcpt_estimator *est /* may be NULL */,
                           const mcpt_render_params *params, uint32_t *seeds_dev, float *hist_dev,
                           int32_t *count_dev, void *stream);

/* Tile-subset render (opt-in, no reference counterpart; ABI 5: a new struct
 * with new entry points).  k_render hands out work by 8x8
 * tile; a tile set names the tiles a call renders.  Tiles are the image's,
 * row-major over ceil(W/8) x ceil(H/8); an edge tile's pixels outside the image
 * do not exist.
 *
 * mcpt_render_frames_tiles is mcpt_render_frames_est with a tile set.
 *  - tiles == NULL: mcpt_render_frames_est's call bit for bit (that entry point
 *    is this one with NULL).  A mask without a zero byte: the same.
 *  - a mask of zero bytes only: MCPT_OK; no launch is enqueued, no state is
 *    touched, and mcpt_stats.launches of the call is 0.
 *  - otherwise every pixel of a tile whose byte is nonzero is advanced exactly
 *    as the whole-image call advances it: seeds, hist and count come out with
 *    the whole-image call's bits (a pixel draws from its own seed chain alone).
 *    The seeds, hist and count words of every other pixel are neither read nor
 *    written; with stats on, mcpt_stats and mcpt_set_pixel_segments count the
 *    active pixels' work alone.
 * MCPT_ERR_ARG, and nothing is touched: mask == NULL in a non-null set,
 * n_tiles != ceil(W/8) * ceil(H/8), params->stripe_count != 1 (tile ids are
 * plain image tiles; a striped subset is not defined), and everything
 * mcpt_render_frames_est refuses.  pad is ignored.
 * mask is host memory, read before the call returns and not kept.  The
 * library derives the list of active tiles itself (in range and distinct by
 * construction: two entries for one pixel would put two lanes on its hand-off
 * chain), in a context-owned device buffer written on `stream` behind the
 * work already enqueued there; like the context's other launch buffers it
 * serves the calls of one stream at a time.  The list's order is speed only:
 * the view's dearest-first tile order filtered by the mask where the call has
 * one, else ascending.  The primary-hit cache stays whole-view: a subset call
 * reads it by pixel id and, where a whole-image call would build it, builds
 * it for every tile; a jittered or lens call does without it as always.     */
typedef struct mcpt_tile_set {
  const uint8_t *mask; /* host; one byte per 8x8 tile, row-major; nonzero = render */
  int32_t n_tiles;     /* ceil(W/8) * ceil(H/8) */
  int32_t pad;
} mcpt_tile_set;
int mcpt_render_frames_tiles(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_camera *cam,
                             const mcpt_lens *lens /* may be NULL */, const mcpt_estimator *est /* may be NULL */,
                             const mcpt_tile_set *tiles /* may be NULL */, const mcpt_render_params *params,
                             uint32_t *seeds_dev, float *hist_dev, int32_t *count_dev, void *stream);

/* Half-buffer noise estimate (opt-in, no reference counterpart; Dammertz et
 * al. 2010).  A render's frames go alternately into two
 * histories A and B (hist + count each, as the render calls keep them); their
 * difference relative to the brightness estimates the error of their mean.
 * Both calls read their inputs only, are ordered on `stream`, asynchronous,
 * and give the same bits for the same inputs.  fp32 throughout; a / b below is
 * the device's 2.5-ulp division, sqrt its square root (1 ulp), fma one rounding.
 *
 * Merged mean of a pixel, per channel c of x, y, z, with fA = (float)nA,
 * fB = (float)nB:   nB == 0: A's four words, bit for bit;  nA == 0: B's;
 *   both 0: four zero words (the first rule);  else
 *   m.c = fma(fA, A.c, fB * B.c) / (float)(nA + nB),   m.w = 0.
 * Merged count nA + nB.  mcpt_merge_halves writes both for n pixels.
 *
 * Pixel error, with m as above:
 *   d = (|A.x - B.x| + |A.y - B.y|) + |A.z - B.z|
 *   s = fmax(((floor + m.x) + m.y) + m.z, floor)     (the fmax never acts on means >= 0)
 *   e = (0.5f * d) / sqrt(s),      e = +inf where nA == 0 or nB == 0.
 * Tile error (mcpt_tile_error, one float per 8x8 tile, row-major as above):
 * the tile's pixels outside the image count 0; the 64 values are summed by the
 * butterfly v[k] += v[k ^ 32], then ^ 16, 8, 4, 2, 1 (k = row * 8 + column in
 * the tile), and the sum is divided by (float)(pixels inside the image).
 * Every term is non-negative, so the result is within 28 * 2^-24 relative of
 * the real-arithmetic value (DESIGN.md 3.19 adds it up); an inf or NaN input
 * carries through.
 * MCPT_ERR_ARG: a null pointer, width or height <= 0 (n < 0), floor not
 * finite or <= 0, a hist pointer not 16-byte aligned.  n == 0 does nothing.  */
int mcpt_tile_error(mcpt_ctx *ctx, int32_t width, int32_t height, const float *histA_dev, const int32_t *countA_dev,
                    const float *histB_dev, const int32_t *countB_dev, float floor, float *err_dev /* n_tiles */,
                    void *stream);
int mcpt_merge_halves(mcpt_ctx *ctx, const float *histA_dev, const int32_t *countA_dev, const float *histB_dev,
                      const int32_t *countB_dev, int64_t n, float *hist_out_dev, int32_t *count_out_dev,
                      void *stream);

/* Launch-plan knobs (speed only), kept in the context; NULL resets them.  */
int mcpt_set_tuning(mcpt_ctx *ctx, const mcpt_tuning *tuning);
int mcpt_get_tuning(mcpt_ctx *ctx, mcpt_tuning *out);
/* Forget the primary-hit cache (mcpt_tuning.primary_cache): the next render
 * call traces or recomputes its primary hits itself (bench.py's timed call). */
int mcpt_drop_caches(mcpt_ctx *ctx);
/* The search-tree node format of the last render call: 0 the 128-B nodes (and
 * NOPRUNE's binary tree), 1 the 64-B quantized nodes (mcpt_stats.quantized),
 * 2 the 96-B exact nodes.  A new entry point; no struct changes.            */
int mcpt_get_node_format(mcpt_ctx *ctx, int32_t *out);

/* Per-image state in HBM for C/C++ hosts that do not manage device memory
 * themselves: the reference's randBuffer (scenebuild.cpp:113-120),
 * frameBuffer and sampleCount (colorout.cpp), W*H each.  create copies the
 * host seeds in and zeroes mean and count; buffers() returns the device
 * pointers mcpt_render_frames takes; download copies any of them back to
 * host arrays (NULL skips one) after the context's work on `stream` is done
 * (ColorOut's dump read, colorout.cpp:55-68).                            */
typedef struct mcpt_state mcpt_state;
int mcpt_state_create(mcpt_ctx *ctx, int32_t width, int32_t height, const uint32_t *seeds_host, mcpt_state **out);
int mcpt_state_buffers(mcpt_state *st, uint32_t **seeds_dev, float **hist_dev, int32_t **count_dev);
int mcpt_download(mcpt_ctx *ctx, const mcpt_state *st, float *hist_rgba, int32_t *count, uint32_t *seeds,
                  void *stream);
/* Checkpoint / resume: mcpt_upload writes host arrays (NULL skips one) into
 * the state, ordered on `stream` before later renders; a state saved with
 * mcpt_download and uploaded into a fresh one continues the render exactly
 * (the per-pixel seed chain, mean and count are the whole of it). */
int mcpt_upload(mcpt_ctx *ctx, mcpt_state *st, const float *hist_rgba, const int32_t *count, const uint32_t *seeds,
                void *stream);
int mcpt_state_destroy(mcpt_state *st);

/* Wavefront kernels on the reference's AoS records, one per reference
 * kernel, for drop-in use and kernel-level parity:                       */
/* rayGenerator.cl generateRay (W x H NDRange)                            */
int mcpt_generate_rays(mcpt_ctx *ctx, const mcpt_camera *cam, int32_t width, int32_t height,
                       mcpt_ray *rays_dev, void *stream);
/* The same with a jittered render's sub-pixel offsets (mcpt_render_frames,
 * params->jitter): pixel (idx, idy) takes its two draws from, and writes the
 * advanced seed back to, seeds_dev[idy * width + idx].                     */
int mcpt_generate_rays_jittered(mcpt_ctx *ctx, const mcpt_camera *cam, int32_t width, int32_t height,
                                uint32_t *seeds_dev, mcpt_ray *rays_dev, void *stream);
/* mcpt_generate_rays_jittered plus the lens of mcpt_render_frames_lens: four
 * draws a pixel (jx, jy, r1, r2).  A null lens or radius 0: the jittered
 * call's bits, two draws.  A bad lens: MCPT_ERR_ARG.                        */
int mcpt_generate_rays_lens(mcpt_ctx *ctx, const mcpt_camera *cam, const mcpt_lens *lens, int32_t width,
                            int32_t height, uint32_t *seeds_dev, mcpt_ray *rays_dev, void *stream);
/* intersect.cl intersectRays (tmin = EPSILON 1e-3, oclbasic.h:193)
 * Arbitrary rays (a unit direction is the callers' convention, not a
 * requirement).  MCPT_MODE_EXACT gives the reference kernel's t, normal,
 * point and material_id for every live ray whose direction components are
 * finite: a ray with a component 0 < |d| < 2^-126 (denormal, not zero), the
 * one class on which the hoisted rcp(d) differs from the reference's
 * division, is searched with the literal division.
 * Measured up to |d| = 1 only: a component above 2^126, whose reciprocal is
 * denormal, is outside what tests/test_gpu_intersect_edges.py shoots.      */
int mcpt_intersect(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_ray *rays_dev,
                   int64_t n, mcpt_hit *hits_dev, float tmin, int32_t mode, void *stream);
/* shade.cl shade (-D MAX_DEPTH)                                           */
int mcpt_shade(mcpt_ctx *ctx, const mcpt_scene *scene, mcpt_ray *rays_dev,
               const mcpt_hit *hits_dev, float *color_dev, uint32_t *seeds_dev, int64_t n,
               int32_t max_depth, void *stream);
/* mcpt_shade with mcpt_estimator's Russian roulette, on plain and textured
 * scenes alike.  rr_depth = 0: mcpt_shade's bits; < 0 or > 65535:
 * MCPT_ERR_ARG.                                                           */
int mcpt_shade_est(mcpt_ctx *ctx, const mcpt_scene *scene, mcpt_ray *rays_dev,
                   const mcpt_hit *hits_dev, float *color_dev, uint32_t *seeds_dev, int64_t n,
                   int32_t max_depth, int32_t rr_depth, void *stream);
/* history.cl func (-D MAX_ATTEMPT): running mean of non-zero samples      */
int mcpt_accumulate(mcpt_ctx *ctx, float *color_dev, float *hist_dev, int32_t *count_dev,
                    int64_t n, int32_t max_attempt, void *stream);
/* The same with mcpt_estimator's counted history: the running mean of every
 * sample, the all-zero ones included.                                      */
int mcpt_accumulate_all(mcpt_ctx *ctx, float *color_dev, float *hist_dev, int32_t *count_dev,
                        int64_t n, int32_t max_attempt, void *stream);
/* testkernel.cl func, ColorOut's display pass (colorout.cpp:58-70): per
 * pixel (pow(r, 1/2.2f), pow(g, 1/2.2f), pow(b, 1/2.2f), 0) into a float4
 * buffer (the reference writes it to its RGBA32F GL texture).  The reference
 * shows the current frame's colours before MAX_ATTEMPT and frameBuffer (the
 * running mean, mcpt_state's hist) after.  n = pixels; may run in place.    */
int mcpt_gamma_preview(mcpt_ctx *ctx, const float *color_dev, float *out_dev, int64_t n, void *stream);

/* Opt-in denoise post-pass (no reference counterpart): a
 * count-aware, geometry-guided a-trous filter of the accumulated image.  The
 * history keeps the mean over a pixel's NON-ZERO samples, so a short render
 * is mostly count-0 pixels; every tap is weighted by its count, so such a
 * pixel carries no information instead of carrying black.
 *  hits_dev   width*height first hits of the view, mcpt_generate_rays then
 *             mcpt_intersect in the caller's render mode (the corner ray's,
 *             also for a jittered render);
 *  hist_dev, count_dev   the image state, read only;
 *  out_dev    width*height float4, never hist_dev.
 * A pixel is filtered when its first hit is a hit (t < FLT_MAX) with
 * material_id < n_mats on a MCPT_DIFFUSE or MCPT_GLOSSY material; every other
 * pixel comes out as hist_dev's float4 bit for bit and is never a tap.  A
 * filtered pixel p starts from c = hist.xyz, W = (float)count and takes, for
 * i = 0 .. iterations-1 with s = 2^i, over the 5x5 taps q = p + s*(dx, dy)
 * that lie inside the image, are filtered, have W_q > 0 and p's material id,
 *   w_q = k[dx] k[dy] W_q exp(-|n_p - n_q|^2 / sigma_normal^2
 *                             - (n_p . (x_q - x_p))^2 / (sigma_plane D)^2
 *                             - |c_p - c_q|^2 / (sigma_color 2^-i)^2),
 * k = (1, 4, 6, 4, 1) / 16, D = the length of the scene root box's diagonal,
 * the colour term only with sigma_color > 0 and W_p > 0; then c = sum(w_q c_q)
 * / sum(w_q), W = sum(w_q), or, when no tap counts, c unchanged and W = 0.
 * It comes out as (c, 0).  iterations = 0 copies hist_dev.  The call writes
 * out_dev and context-owned scratch (64 B per pixel, grown on demand) and
 * nothing else: not hist, count or seeds, nor any cache of the context, so a
 * render continued afterwards is unaffected.  Stream-ordered and asynchronous.
 * MCPT_ERR_ARG: a null pointer, a non-positive size, iterations outside 0..8,
 * a sigma that is not finite, sigma_normal or sigma_plane <= 0, sigma_color
 * < 0, out_dev == hist_dev, hits_dev / hist_dev / out_dev not 16-B aligned.  */
typedef struct mcpt_denoise_params {
  int32_t iterations;      /* 0..8; 0 copies hist                        */
  float sigma_normal;      /* > 0                                          */
  float sigma_plane;       /* > 0, as a fraction of the scene diagonal     */
  float sigma_color;       /* >= 0; 0: no colour term                      */
} mcpt_denoise_params;
int mcpt_denoise(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_hit *hits_dev,
                 const float *hist_dev, const int32_t *count_dev,
                 int32_t width, int32_t height,
                 const mcpt_denoise_params *params, float *out_dev, void *stream);

/* Opt-in environment lighting (no reference counterpart): what
 * a ray that leaves the scene picks up.  The reference, and a scene without
 * an environment, give such a ray black (shade.cl:89-93).
 * An environment is a scale (r, g, b: finite, >= 0; scale[3] is ignored), an
 * optional lat-long map and a rotation rotate_deg (finite, degrees about +Y).
 * The map is width x height RGB float texels, 3 floats each, rows in file
 * order with row 0 the top (+Y), every texel finite and >= 0, 1 <= width,
 * height and width * height <= 2^26; map_rgb NULL: no map, width and height
 * ignored.  For a unit ray direction d, in real arithmetic (the kernels
 * evaluate it in fp32, tests/env_ref.py restates it in float64):
 *   d' = (c d.x + s d.z, d.y, -s d.x + c d.z), c = cos(rotate), s = sin(rotate)
 *        computed in double on the host and rounded to float once;
 *   u = 0.5 + atan2(d'.x, -d'.z) / (2 pi),  v = acos(clamp(d'.y, -1, 1)) / pi;
 *   x = u * width - 0.5,  y = v * height - 0.5,  i0 = floor(x),  j0 = floor(y),
 *   fx = x - i0, fy = y - j0;  T = the bilinear mix of texels (i0, j0),
 *   (i0 + 1, j0), (i0, j0 + 1), (i0 + 1, j0 + 1) with weights (1 - fx)(1 - fy),
 *   fx (1 - fy), (1 - fx) fy, fx fy, columns taken modulo width, rows clamped
 *   to [0, height - 1];
 *   L = (scale.r T.r, scale.g T.g, scale.b T.b, 0).
 * Without a map L = (scale.r, scale.g, scale.b, 0) and no trigonometry runs.
 * A path whose segment misses ends as it does without an environment, but its
 * colour is color * L instead of 0, in mcpt_render_frames and in mcpt_shade.
 * L.w = 0 on purpose: a zero-radiance environment gives the all-zero sample
 * the history skips, so scale = 0 renders the bits of no environment.  The
 * depth cap, the history rule, max_attempt, the seed chain (the lookup draws
 * nothing), the hand-off and the primary-hit records are untouched.
 * mcpt_scene_set_environment copies and uploads the map (float4 texels in
 * HBM), replacing a previous environment of the scene; env NULL clears it (the
 * bits of a scene that never had one).  mcpt_scene_destroy frees the map.  The
 * context's primary-hit cache stays valid: it holds hits, not radiance.  It
 * waits for work already enqueued on the scene's GPU before it frees a
 * previous map.  MCPT_ERR_ARG (the environment unchanged): a null context or
 * scene, a scale or rotate_deg that is not finite, a negative scale, a map
 * with a dimension < 1, more than 2^26 texels, or a texel that is negative
 * or not finite.                                                          */
typedef struct mcpt_environment {
  float scale[4];
  const float *map_rgb;             /* host, width * height * 3 floats, or NULL */
  int32_t width, height;
  float rotate_deg;
} mcpt_environment;
int mcpt_scene_set_environment(mcpt_ctx *ctx, mcpt_scene *scene, const mcpt_environment *env);
/* L of the scene's environment for n rays (their direction's xyz, taken as
 * unit vectors) into out_rgba_dev, n float4; zeros when the scene has no
 * environment.  Both arrays on the device, 16-B aligned.  Stream-ordered and
 * asynchronous.  With mcpt_generate_rays: the view's background plate.     */
int mcpt_env_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const mcpt_ray *rays_dev, int64_t n,
                  float *out_rgba_dev, void *stream);

/* Opt-in smooth shading from interpolated vertex normals (no reference
 * counterpart).  The reference, and a scene without vertex
 * normals, shade every hit with its triangle's packed face normal ng.
 *
 * mcpt_vertex_normals generates them on the host from n PACKED triangles
 * (mcpt_pack_triangles) into vn, n x 3 corners x 3 floats; crease_deg in
 * [0, 180].  Normative (tests/smooth_ref.py restates it in float64):
 *   - corners are welded by the exact bits of their position, -0 as +0;
 *   - corner k of triangle i takes the sum, in double and in ascending
 *     triangle index, of angle_j * ng_j over the corners of triangles j at the
 *     same position whose ng_j is bit-equal to ng_i or, for crease_deg > 0, has
 *     dot(ng_i, ng_j) >= cos(crease) (the dot in double); angle_j = triangle
 *     j's interior angle there, atan2(|e x f|, e . f) of its two edges;
 *   - the sum is normalised in double and rounded to float once;
 *   - a triangle whose ng is not finite or whose length is not within 1e-3 of
 *     1 (degenerate) contributes nowhere and keeps ng at its corners;
 *   - a corner whose contributing normals are all bit-equal to ng_i, or whose
 *     sum is shorter than 1e-12, takes ng_i bit for bit: a cube, and any mesh
 *     at crease 0, comes out exactly flat.
 * An oppositely wound neighbour has dot ~ -1 and is excluded like any crease.
 * The weld is a sort of the corners by position: O(n log n).  A vertex shared
 * by m corners costs O(m) when all their face normals lie within half the
 * crease angle of their mean (a pole, a flat fan: every pair is then inside
 * the crease and every corner takes the one sum, the same value the pairwise
 * rule gives), else m^2 pair tests; MCPT_ERR_LIMIT when such a vertex has
 * more than 65536 corners.
 *
 * mcpt_load_obj_normals reads authored normals: the `vn` records and the
 * third index of "v/vt/vn" and "v//vn" corners (negative indices count back
 * from the records read so far), with mcpt_load_obj's fan triangulation and
 * triangle order.  has[i] = 1 when all three corners of triangle i name a vn
 * record of finite, non-zero length; vn[9 i ..] then holds them normalised in
 * double, else zeros.  vn and has NULL: *n_tris = the count only; otherwise
 * *n_tris is the buffers' capacity in triangles on entry.  MCPT_ERR_PARSE: a
 * vn index past the file's records or before the first, a face index of 0.
 * mcpt_obj_normals_from_text is the same parser on `len` bytes in memory
 * (it reads exactly those bytes).
 *
 * mcpt_scene_set_vertex_normals(ctx, scene, vn): vn = n_tris x 9 floats on
 * the host in the upload's triangle order, n_tris the scene's count; every
 * normal finite with length within 1e-3 of 1, except in a triangle whose
 * three normals are bit-equal to its packed normal (flat: never
 * interpolated).  Uploads 48 B per triangle (two copies, 48 B per triangle
 * and 192 B per search-tree node, in a scene that has the 96-B nodes),
 * replacing the scene's previous ones; vn NULL clears them (the bits of a
 * scene that never had any).  It waits for work enqueued on the scene's GPU
 * before it frees a previous array, and drops the context's primary-hit
 * cache (its records hold shading normals).  MCPT_ERR_ARG leaves the scene
 * as it was.  mcpt_scene_destroy frees the arrays.
 *
 * The lookup, for a hit at point pt of a ray with direction d on triangle T
 * with rows v0, e1 = v1 - v0, e2 = v2 - v0 and vertex normals n0, n1, n2
 * (fp32 on the device, csrc/mcpt_smooth.h; float64 in tests/smooth_ref.py):
 *   ngf = ng, negated when dot(d, ng) > 0 (the reference's flip,
 *         intersect.cl:23-25);
 *   a triangle whose vertex normals are all bit-equal to ng gives ngf, the
 *   bits a scene without vertex normals gives;
 *   w = pt - v0, d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, w1 = w.e1, w2 = w.e2,
 *   den = d11 d22 - d12^2, b1 = clamp((d22 w1 - d12 w2) / den, 0, 1),
 *   b2 = clamp((d11 w2 - d12 w1) / den, 0, 1), b0 = max(0, 1 - b1 - b2);
 *   ns = normalize(b0 n0 + b1 n1 + b2 n2), negated when dot(ns, ngf) < 0;
 *   ngf instead when den or |ns|^2 is zero or not finite.
 * The result replaces the flipped face normal wherever a hit is shaded:
 * mcpt_render_frames (every material's in.nrm), the primary-hit records,
 * mcpt_intersect's mcpt_hit.normal (so mcpt_shade and mcpt_denoise's guide
 * follow).  No random number is drawn for it and a sampled direction below
 * the geometric surface is traced as sampled.
 * mcpt_render_frames with vertex normals set supports MCPT_MODE_EXACT and
 * MCPT_MODE_NOPRUNE alike.
 *
 * mcpt_shading_normals evaluates the lookup for n queries on the device:
 * tri_ids_dev int32 triangle indices (upload order), points_dev and dirs_dev
 * n float4 (xyz used), out_dev n float4 (w = +-0).  MCPT_ERR_ARG when the
 * scene has no vertex normals; an index outside the scene's triangles gives
 * zeros.  Stream-ordered and asynchronous.                                 */
int mcpt_vertex_normals(const mcpt_triangle *packed_tris, int64_t n, double crease_deg, float *vn);
int mcpt_load_obj_normals(const char *directory, const char *objname, float *vn, uint8_t *has, int64_t *n_tris);
int mcpt_obj_normals_from_text(const char *text, int64_t len, float *vn, uint8_t *has, int64_t *n_tris);
int mcpt_scene_set_vertex_normals(mcpt_ctx *ctx, mcpt_scene *scene, const float *vn);
int mcpt_shading_normals(mcpt_ctx *ctx, const mcpt_scene *scene, const int32_t *tri_ids_dev, const float *points_dev,
                         const float *dirs_dev, int64_t n, float *out_dev, void *stream);

/* Opt-in diffuse texture maps (OBJ `vt`, MTL `map_Kd`; no reference
 * counterpart).  The reference, and a scene without textures,
 * shade the diffuse lobe with the material's kd alone.
 *
 * Normative (fp32 on the device, csrc/mcpt_texture.h; float64 in
 * tests/texture_ref.py).  A scene has a pool of textures, each W x H linear
 * RGB float texels, row 0 the top, every texel finite and >= 0.  Each triangle
 * has three UV pairs and a texture index, or -1: no texture.  For a hit at
 * point pt on triangle T with rows v0, e1 = v1 - v0, e2 = v2 - v0:
 *   b0, b1, b2: the barycentrics of the smooth lookup above (the same rows,
 *     fmas, one v_rcp_f32 and clamps); den zero or not finite: b1 = b2 = 0;
 *   u = b0 u0 + b1 u1 + b2 u2 and v likewise, as fma chains
 *     fma(b2, u2, fma(b1, u1, b0 u0));
 *   u' = u - floor(u), v' = v - floor(v): every texture repeats on both axes;
 *   x = u' W - 0.5, y = (1 - v') H - 0.5 (OBJ's v axis points up), each one
 *     fma; i0 = floor(x), j0 = floor(y), fx = x - i0, fy = y - j0;
 *   bilinear over columns i0, i0 + 1 and rows j0, j0 + 1, BOTH taken modulo W
 *     and H, with the environment map's weights and fma order
 *     (w00 = (1-fx)(1-fy), w10 = fx (1-fy), w01 = (1-fx) fy, w11 = fx fy;
 *     fma(w11, t11, fma(w01, t01, fma(w10, t10, w00 t00)))); a channel whose
 *     four texels are equal is that value exactly (the four fp32 weights sum
 *     to 1 only within an ulp, and a texture of ones must give 1.0f);
 *   Tex = (r, g, b, alpha) (alpha: 1 unless an alpha is set, see the cutouts
 *     below); an untextured triangle gives (1, 1, 1, 1) after one
 *     16-B gather.
 * Shading: kd is replaced by kd * Tex, one multiply per lane, wherever the
 * diffuse lobe of MCPT_DIFFUSE and of MCPT_GLOSSY reads kd.  ks, a light's
 * ka, glass and the environment are untouched; no random number is drawn;
 * x * 1.0f is exact, so a texture of ones, or none, gives the untextured bits.
 * There are no mip levels: minification aliasing at primary hits averages out
 * only with jitter.
 *
 * mcpt_load_obj_uvs reads the `vt` records and the second index of "v/vt" and
 * "v/vt/vn" corners (negative indices count back from the records read so
 * far) with mcpt_load_obj's fan triangulation and triangle order: uv[6 i ..] =
 * (u0, v0, u1, v1, u2, v2), has[i] = 1 when all three corners of triangle i
 * name a finite vt, else zeros.  uv and has NULL: *n_tris = the count only;
 * otherwise *n_tris is the buffers' capacity in triangles on entry.
 * MCPT_ERR_PARSE: a vt index of 0, or one outside the file's records.
 * mcpt_obj_uvs_from_text is the same parser on `len` bytes in memory.
 *
 * mcpt_load_mtl_maps returns each material's map_Kd file name in
 * mcpt_load_obj's material order (the `newmtl` records of the OBJ file's
 * mtllib, in order): '\0'-terminated names back to back, an empty name for a
 * material without a map.  Options before the name (-s, -o, -clamp, -bm, ...)
 * are skipped, not honoured; backslashes become slashes.  Two calls: names
 * NULL gives *n_bytes and *n_materials; otherwise *n_bytes is the buffer's
 * capacity on entry.  mcpt_mtl_maps_from_text is the same on MTL text.
 *
 * mcpt_scene_set_textures(ctx, scene, t): host uv (n_tris x 6) and tri_tex
 * (n_tris) in the upload's triangle order, n_textures images {rgb, width,
 * height} of width * height * 3 floats.  Validated first: UVs of textured
 * triangles finite with |uv| <= 2^20, indices in [-1, n_textures), texels
 * finite and >= 0, sides in 1..16384, at most 2^27 texels in all;
 * MCPT_ERR_ARG leaves the scene as it was.  Uploads float4 texels in one pool
 * and a 32-B record per triangle (a second copy per search-tree slot in a
 * scene that has the 96-B nodes); t NULL clears the textures.  It waits for
 * work enqueued on the scene's GPU before it frees previous arrays and drops
 * the context's primary-hit cache.  mcpt_scene_destroy frees the arrays.
 *
 * With textures set: mcpt_render_frames runs k_render's textured forms (both
 * modes; with or without vertex normals); its primary-hit cache holds each
 * pixel's texture factor beside the hit (16 B per pixel more), the same bits
 * with mcpt_tuning.primary_cache off, auto or always;
 * mcpt_shade multiplies kd by the factor at the hit's triangle_id and point;
 * mcpt_intersect reports the closest hit's triangle in triangle_id in
 * MCPT_MODE_NOPRUNE too (without textures: the reference's last accepted
 * triangle), so that the chain of wavefront kernels looks the texel up on the
 * triangle the point lies on.
 *
 * mcpt_texture_eval evaluates the factor for n queries on the device:
 * tri_ids_dev int32 triangle indices (upload order), points_dev n float4 (xyz
 * used), out_dev n float4.  MCPT_ERR_ARG when the scene has no textures; an
 * index outside the scene's triangles gives zeros.  Stream-ordered.       */
typedef struct mcpt_texture_image {
  const float *rgb; /* width * height * 3, row 0 the top */
  int32_t width, height;
} mcpt_texture_image;
typedef struct mcpt_textures {
  const float *uv;          /* n_tris x 6 */
  const int32_t *tri_tex;   /* n_tris, -1: no texture */
  int32_t n_textures;
  const mcpt_texture_image *images;
} mcpt_textures;
int mcpt_load_obj_uvs(const char *directory, const char *objname, float *uv, uint8_t *has, int64_t *n_tris);
int mcpt_obj_uvs_from_text(const char *text, int64_t len, float *uv, uint8_t *has, int64_t *n_tris);
int mcpt_load_mtl_maps(const char *directory, const char *objname, char *names, int64_t *n_bytes, int64_t *n_materials);
int mcpt_mtl_maps_from_text(const char *text, int64_t len, char *names, int64_t *n_bytes, int64_t *n_materials);
int mcpt_scene_set_textures(mcpt_ctx *ctx, mcpt_scene *scene, const mcpt_textures *textures);
int mcpt_texture_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const int32_t *tri_ids_dev, const float *points_dev,
                      int64_t n, float *out_dev, void *stream);

/* Opt-in alpha cutouts (MTL `map_d`, a texture's alpha channel; no reference
 * counterpart).  Functions and one struct of their own: the
 * ABI revision stays 5.
 *
 * Normative (fp32 on the device, csrc/mcpt_texture.h; float64 in
 * tests/cutout_ref.py).
 * Alpha in the texel pool: each texture of the scene's texture set may carry
 *   an alpha image of its own size, values finite in [0, 1], row 0 the top,
 *   stored in the .w of that texture's float4 texels; a texture without one
 *   has .w = 1.0f in every texel (mcpt_scene_set_textures writes that).  The
 *   scene holds one threshold a0 in (0, 1], default 0.5.
 * Alpha at a hit: Tex.w of the texture lookup above is the same bilinear,
 *   repeating lookup applied to .w, with the same weights and fma order; a
 *   channel whose four texels are equal is that value exactly, so an opaque
 *   texture gives exactly 1.0f; an untextured triangle gives 1.
 * The cutout test is the first thing shading does with a hit of a live ray,
 *   before the material switch and the depth cap, for every material type,
 *   lights included.  A hit is cut when alpha < a0 and the path's pass count c
 *   is below 255.  A cut hit does not shade: the ray goes on from the hit
 *   point, o' = hit point, d' = d bit for bit; the colour, the seed, the depth
 *   and the inside bits are unchanged; c' = c + 1 and no random number is
 *   drawn.  With c == 255 the hit is shaded as if opaque: every path is finite
 *   whatever the geometry.
 * c lives in bits 8..15 of term_depth (origin.w), and the depth in bits 0..7,
 *   while a scene has cutouts; a render or mcpt_shade call with max_depth >
 *   255 on such a scene is MCPT_ERR_ARG.  A scene without cutouts keeps
 *   MCPT_DEPTH_MASK's meaning.
 * So a pass-through ray that then misses takes the environment as any miss
 * does; the next segment starts with the usual tmin of 1e-3; mcpt_intersect is
 * unchanged and reports the closest triangle, cut or not.
 *
 * mcpt_load_mtl_alpha_maps / mcpt_mtl_alpha_maps_from_text are
 * mcpt_load_mtl_maps' twins for `map_d`: the same order, options, slashes and
 * two-call pattern.
 *
 * mcpt_scene_set_texture_alpha(ctx, scene, a): a->alpha[i] is texture i's
 * alpha image (its width * height floats) or NULL for an opaque texture.
 * Validated before anything changes: MCPT_ERR_ARG, with the scene as it was,
 * when the scene has no textures, n_textures is not its texture set's count,
 * a value is outside [0, 1] or not finite, or the threshold is outside (0, 1].
 * a NULL clears: every .w is 1 again and the depth keeps MCPT_DEPTH_MASK.  The
 * call waits for work enqueued on the scene's GPU and drops the context's
 * primary-hit cache, as mcpt_scene_set_textures does; a later
 * mcpt_scene_set_textures (set or clear) drops the alpha.
 *
 * With an alpha set, the primary-hit cache's texture factor holds the primary
 * hit's alpha in .w, so a cached first segment passes through exactly as a
 * traced one does; mcpt_texture_eval's fourth lane is the alpha (1.0f
 * without one).                                                            */
typedef struct mcpt_texture_alpha {
  int32_t n_textures;
  const float *const *alpha; /* n_textures pointers, NULL: opaque */
  float threshold;
  float pad;
} mcpt_texture_alpha;
int mcpt_load_mtl_alpha_maps(const char *directory, const char *objname, char *names, int64_t *n_bytes,
                             int64_t *n_materials);
int mcpt_mtl_alpha_maps_from_text(const char *text, int64_t len, char *names, int64_t *n_bytes, int64_t *n_materials);
int mcpt_scene_set_texture_alpha(mcpt_ctx *ctx, mcpt_scene *scene, const mcpt_texture_alpha *a);

/* Opt-in bump and normal maps (MTL `map_Bump`, `bump`, `norm`; no reference
 * counterpart).  The reference, and a scene without maps,
 * shade a hit with its face normal (or, with vertex normals, the interpolated
 * one).
 *
 * Normative (fp32 on the device, csrc/mcpt_bump.h; float64 in
 * tests/bump_ref.py).  A scene has a second pool of maps, each W x H
 * tangent-space normals (mx, my, mz) as float texels, row 0 the top, every
 * texel unit within 1e-3 with mz > 0; red is +u and green is +v, where OBJ's v
 * points up (the "Y+" convention).  Each triangle has three UV pairs and a map
 * index, or -1: unmapped.
 * At set time, on the host in double, with e1 = v1 - v0, e2 = v2 - v0 (the
 * uploaded rows), du1 = u1 - u0, dv1 = v1 - v0 and du2, dv2 likewise:
 *   det = du1 dv2 - du2 dv1; T = (dv2 e1 - dv1 e2) / det;
 *   B = (du1 e2 - du2 e1) / det; t = normalize(T), rounded once;
 *   h = +1 when dot(cross(ng, T), B) >= 0, else -1 (ng: the packed face
 *   normal); det zero or not finite, or T zero or not finite: unmapped.
 * At a shaded hit with ray direction d, N the normal that would be shaded
 * without maps (the ray-facing result of the smooth lookup above, or the
 * flipped face normal):
 *   1. m = (mx, my, mz): the barycentrics, u', v', x, y and the bilinear filter
 *      with wrap of the texture lookup above, bit for bit (the rule that a
 *      channel whose four texels are equal is that value exactly included),
 *      over the normal pool;
 *   2. an unmapped triangle gives N bit for bit after one 16-B gather; so does
 *      mx == 0 && my == 0;
 *   3. f = dot(N, ng) < 0 ? -1 : +1; nt = dot(N, t); tp = fma(-nt, N, t) per
 *      component; |tp|^2 zero or not finite gives N; T' = normalize(tp);
 *      B' = (h f) cross(N, T');
 *   4. n = fma(mz, N, fma(my, B', mx T')) per component; |n|^2 zero or not
 *      finite gives N; n' = normalize(n); a non-finite n' gives N; dot(n', d)
 *      >= 0 (turned away from the viewer) gives N; n'.w keeps N.w's bits.
 * dot, cross and normalize are those of the shading code (fma chains, one
 * v_rsq_f32).  No random number is drawn.  n' replaces the shading normal for
 * every material, as smooth normals do.
 *
 * mcpt_load_mtl_bump_maps returns, per material in mcpt_load_obj's material
 * order, the map's file name ('\0'-terminated, back to back; empty: none), its
 * kind (MCPT_BUMP_NORMAL for `norm`, MCPT_BUMP_HEIGHT for `map_Bump`,
 * `map_bump` or `bump`, MCPT_BUMP_NONE) and its `-bm` value (default 1).
 * Other options are skipped; `norm` wins over a height map whatever their
 * order; backslashes become slashes.  Two calls: names NULL gives *n_bytes and
 * *n_materials; otherwise *n_bytes is the name buffer's capacity and kinds and
 * bm hold *n_materials entries on entry.  mcpt_mtl_bump_maps_from_text is the
 * same on MTL text.
 *
 * mcpt_scene_set_normal_maps(ctx, scene, m): host uv (n_tris x 6) and tri_map
 * (n_tris) in the upload's triangle order, n_maps images {xyz, width, height}
 * of width * height * 3 floats.  Validated first: UVs of mapped triangles
 * finite with |uv| <= 2^20, indices in [-1, n_maps), texels as above, sides in
 * 1..16384, at most 2^27 texels in all (checked from the sizes before a texel
 * is read); MCPT_ERR_ARG leaves the scene as it was.  Uploads float4 texels in
 * one pool and a 48-B record per triangle (a second copy per search-tree slot
 * in a scene that has the 96-B nodes); m NULL clears the maps.  It waits for
 * work enqueued on the scene's GPU before it frees previous arrays and drops
 * the context's primary-hit cache.  mcpt_scene_destroy frees the arrays.
 *
 * With maps set: mcpt_render_frames runs k_render's mapped forms (both modes;
 * with or without vertex normals and textures); its primary-hit cache holds
 * n' as the finished normal, the same bits with mcpt_tuning.primary_cache off,
 * auto or always; mcpt_intersect writes n' to mcpt_hit.normal and reports the
 * closest hit's triangle in both modes, as on a textured scene, so mcpt_shade
 * and the denoiser's guide follow.
 *
 * mcpt_bump_eval evaluates n' for n queries on the device: tri_ids_dev int32
 * triangle indices (upload order), points_dev, dirs_dev and normals_dev n
 * float4 each (xyz used; normals_dev is N, .w kept), out_dev n float4.
 * MCPT_ERR_ARG when the scene has no maps; an index outside the scene's
 * triangles gives zeros.  Stream-ordered.                                  */
#define MCPT_BUMP_NONE 0
#define MCPT_BUMP_HEIGHT 1
#define MCPT_BUMP_NORMAL 2
typedef struct mcpt_normal_map_image {
  const float *xyz; /* width * height * 3, row 0 the top */
  int32_t width, height;
} mcpt_normal_map_image;
typedef struct mcpt_normal_maps {
  const float *uv;          /* n_tris x 6 */
  const int32_t *tri_map;   /* n_tris, -1: unmapped */
  int32_t n_maps;
  const mcpt_normal_map_image *images;
} mcpt_normal_maps;
int mcpt_load_mtl_bump_maps(const char *directory, const char *objname, char *names, int32_t *kinds, float *bm,
                            int64_t *n_bytes, int64_t *n_materials);
int mcpt_mtl_bump_maps_from_text(const char *text, int64_t len, char *names, int32_t *kinds, float *bm,
                                 int64_t *n_bytes, int64_t *n_materials);
int mcpt_scene_set_normal_maps(mcpt_ctx *ctx, mcpt_scene *scene, const mcpt_normal_maps *maps);
int mcpt_bump_eval(mcpt_ctx *ctx, const mcpt_scene *scene, const int32_t *tri_ids_dev, const float *points_dev,
                   const float *dirs_dev, const float *normals_dev, int64_t n, float *out_dev, void *stream);

/* Counters of the last render call (segments etc. need stats enabled);
 * waits for that call's work to finish.                                   */
int mcpt_set_stats(mcpt_ctx *ctx, int32_t enabled);
int mcpt_get_stats(mcpt_ctx *ctx, mcpt_stats *out);

/* Diagnostics: with stats on, every render call adds each pixel's segments
 * (the chain of work its frames are, one sequential seed chain per pixel)
 * into counts_dev[y * width + x] and the k_render loop iterations its lane
 * spent on it into iters_dev (width*height u32 each on the device, zeroed by
 * the caller; either may be NULL); NULL, NULL stops it.  n_pixels is the
 * buffers' capacity in pixels: a call whose image has more pixels collects
 * nothing (never writes past them).                                        */
int mcpt_set_pixel_segments(mcpt_ctx *ctx, uint32_t *counts_dev, uint32_t *iters_dev, int64_t n_pixels);
/* The primary-hit pass's per-pixel traversal cost of the cached view (loop
 * iterations of k_render's PRIM form, or node steps + triangle tests of
 * k_primary), width*height u32 to the host; *n = 0 when no cache is held.
 * Pixels outside the cached call's own row stripes read 0.                */
int mcpt_get_primary_cost(mcpt_ctx *ctx, uint32_t *out, int64_t cap, int64_t *n);

/* Diagnostics (MCPT_PHASE_TIMING builds, libmcpt_hip_timing.so): the
 * timeline of every 64-lane wave of the last render call's last k_render
 * launch, 8 words each: start, the first moment one of its lanes found every
 * work queue dry, end, the latest start of a queue entry (s_memrealtime
 * ticks, 100 MHz, chip-wide clock), loop iterations, entries started,
 * lane-iterations spent waiting for a pixel's previous block, XCD.  Waits
 * for the call.  Release builds log nothing: *n_workgroups = 0.  out may be
 * NULL to ask for the count.                                               */
int mcpt_get_wave_log(mcpt_ctx *ctx, uint64_t *out, int64_t cap_workgroups, int64_t *n_workgroups);

/* Diagnostics (MCPT_PHASE_TIMING builds): for a render call of one launch
 * with at most 16 M (pixel, block) entries, the low 32 bits of the 100 MHz
 * s_memrealtime clock at each entry's claim, start (its pixel's previous
 * block published) and end, 3 words per entry at (pixel * blocks + block) * 3
 * (0: never claimed).  *n_entries = pixels * blocks (0 otherwise, and on
 * release builds).  Waits for the call.                                    */
int mcpt_get_entry_log(mcpt_ctx *ctx, uint32_t *out, int64_t cap_entries, int64_t *n_entries, int32_t *blocks);

/* HLBVH::build (MCPT/BVH/hlbvh.cpp:92-200) on the GPU: triangles and the
 * 2n-1 output nodes are DEVICE pointers; the tree is bit-identical to
 * mcpt_build_hlbvh's (finite vertices).  Synchronises `stream`.           */
int mcpt_build_hlbvh_device(const mcpt_triangle *tris_dev, int64_t n, mcpt_bvh_node *nodes_dev, void *stream);

/* TreeletBVH<CPU> (MCPT/BVH/treeletBVH.cpp:343-372, the reference's
 * "bvhtype": "treelet", scenebuild.cpp:70-73) on the GPU, in place on a
 * DEVICE array of 2n-1 nodes as mcpt_build_hlbvh[_device] lays them out:
 * Karras-Aila treelets of up to 7 leaves rebuilt bottom-up with the
 * reference's heap order, subset DP and refit, bit-identical to the
 * reference's sequential pass.  MCPT_ERR_ARG when the reference's own SAH
 * recursion would not terminate on the tree (treeletBVH.cpp:327 quirk).
 * Synchronises `stream`.                                                  */
int mcpt_treelet_device(mcpt_bvh_node *nodes_dev, int64_t n_nodes, void *stream);

/* TreeletBVH<GPU> (MCPT/BVH/treeletBVH.cpp:413-438 + kernels/treeletBVH.cl:230-531):
 * the GPU treelet kernel the reference runs on a fresh HLBVH for EVERY
 * bvhtype before rendering (SceneCL's ctor falls through into its GPUBVH
 * block, scenebuild.cpp:66-95), so the tree its intersect kernel reads.  In
 * place on a DEVICE array of 2n-1 nodes in the HLBVH layout (internal nodes
 * [0, n-2], leaves [n-1, 2n-2]).  The kernel's warp-synchronous behaviour is
 * restated deterministically: its pickNode argmax, lockstep
 * reductions and tie stores (highest lane lands), its refit SAH without
 * /rootArea (treeletBVH.cl:524-525), FP as ROCm's OpenCL compiler builds it
 * for gfx950.  Parity unpinned (treeletBVH.cl:80-81 does not compile).
 * Synchronises `stream`.                                                  */
int mcpt_treelet_gpu_device(mcpt_bvh_node *nodes_dev, int64_t n_nodes, void *stream);
/* Same on a HOST array, the way the reference host uses it on its own node
 * vector (upload, restructure, read back; scenebuild.cpp:89-94,
 * bvhtest.cpp:503-511), on the calling thread's current device.           */
int mcpt_treelet_gpu(mcpt_bvh_node *nodes, int64_t n_nodes);

/* BVH quality metrics of "testbvh" (bvhtest.cpp:448-530), on the GPU.
 * EPO_GPU (bvhtest.cpp:288-321 + kernels/EPO.cl:133-197): per-triangle EPO
 * area and triangle area into the caller's DEVICE arrays (n_tris floats
 * each), bit-identical to the reference kernel; *epo (optional) = their
 * double sums in index order, divided, as the float EPO_GPU returns.
 * *clip_overflows (optional) counts triangles whose clipped polygon exceeds
 * the reference kernel's 8-entry arrays (undefined behaviour there).       */
int mcpt_bvh_epo_device(const mcpt_bvh_node *nodes_dev, const mcpt_triangle *tris_dev, int64_t n_tris,
                        float *epo_dev, float *area_dev, double *epo, uint64_t *clip_overflows, void *stream);
/* LCV (bvhtest.cpp:324-444): leaves hit per pixel-centre camera ray into
 * counts_dev (width*height u32, index i*height + j as the reference pushes
 * its rays), *lcv (optional) = their standard deviation (float result).    */
int mcpt_bvh_lcv_device(const mcpt_bvh_node *nodes_dev, int64_t n_nodes, const mcpt_camera *cam,
                        int32_t width, int32_t height, uint32_t *counts_dev, double *lcv, void *stream);

/* Streaming-read bandwidth of this GPU's HBM (GB/s, best of 5 reads of
 * `bytes` after a warm-up): the measured roofline denominator SURVEY.md
 * §8(d) asks for next to the 8 TB/s spec.                                 */
int mcpt_measure_read_bw(mcpt_ctx *ctx, int64_t bytes, double *gbps);

/* Counter calibration for the roofline: gathers every
 * record of a fresh table_bytes table (a power of two, evicted from the
 * Infinity Cache first) once, in scrambled order, as whole record_bytes
 * records (64: k_render's triangles, 128: its nodes) with one 16-B load per
 * lane and slot.  The known byte count is table_bytes; rocprofv3's
 * FETCH_SIZE for kernel k_gather_probe against it gives the counter's scale
 * for this access shape.  *ms = the kernel's device time.                  */
int mcpt_gather_probe(mcpt_ctx *ctx, int32_t record_bytes, int64_t table_bytes, double *ms);

/* Device self-check of the inline sin/cos used by randomDirection
 * (shade.cl:40-59) against the ocml library calls the reference kernel
 * makes: mismatching bit patterns over the 32768 angles 2*pi*r/32768 and
 * over every float in [0, 8). Both counts are 0 on a correct build.       */
int mcpt_selfcheck_trig(mcpt_ctx *ctx, int64_t *angle_mismatches, int64_t *range_mismatches);
/* The Phong lobe's pow restatement (cl_pow_lobe, mcpt_refmath.h) against
 * ocml's pow_f32 over every float of its domain (0, 1 + 2^-10], for each of
 * the n exponents ys (the scenes' Ns); *mismatches = differing results.      */
int mcpt_selfcheck_pow(mcpt_ctx *ctx, const float *ys, int32_t n, int64_t *mismatches);

#ifdef __cplusplus
}
#endif
#endif /* MCPT_HIP_H */
