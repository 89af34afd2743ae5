/*
 * pt_abi.h -- C-ABI drop-in boundary of the MI355X progressive path tracer.
 *
 * The reference has no plugin/FFI API; its de-facto boundary is the GL
 * contract around pass1.draw() (OpenglRayTracing/main.cpp:558-603,
 * DisneyBRDF/main.cpp:558-603, ImportanceSampling_LowDiscrepancySequence/
 * main.cpp:659-709). Each entry point below replaces one piece of that
 * contract; the reference call it replaces is cited on each declaration.
 *
 * Conventions
 *  - Return codes: 0 = OK, negative = PT_E_* (no exit(), unlike the reference's
 *    exit(-1) at OpenglRayTracing/main.cpp:175,214,225,269).
 *  - The caller owns host arrays; the library owns device buffers.
 *  - One host thread per pt_ctx; calls are stream-ordered and synchronous on
 *    return unless the name ends in _async.
 *  - Images are row-major, row 0 = the bottom row (GL window coordinates,
 *    pass1.fsh pix.y) for the GL integrators, row 0 = the top row for
 *    PT_BASIC_CPU_COMPAT (BasicRayTracingWithC++/main.cpp:364-370).
 */
#ifndef PT_ABI_H
#define PT_ABI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 13 /* 2: in-process multi-GPU fields at the end of pt_config / pt_frame_stats;
                             3: scene-upload fields at the end of pt_frame_stats, pt_build_bvh_device;
                             4: BASIC shapes as doubles, its double image, the replayed random stream;
                             5: the displayed frame of a screen-tile split (pt_display_*);
                             6: batches of frames (pt_render_frames_async, pt_config.frame_batch,
                                pt_frame_stats.frames), pt_config.hw_queues;
                             7: pt_unpack_ranks (every other rank's f32 gather in one launch);
                                PT_FLAG_WAVEFRONT retired; pt_frame_stats.env_compact, tree4_nodes;
                             8: guide buffers and the edge-avoiding a-trous denoised display (pt_render_guides,
                                pt_denoise, pt_display_denoised); no existing struct changes;
                             9: the running mean reprojected across camera moves (pt_temporal_resolve,
                                pt_temporal_commit, pt_display_resolved) and pt_denoise_from; no existing
                                struct changes;
                             10: per-pixel sample moments (PT_FLAG_MOMENTS, pt_download_moments) and the
                                variance-guided filter (pt_denoise_var); no existing struct changes;
                             11: diagnostics only: pt_fmath_* ids 7-10 (the float approximations and
                                ptm_sincosf) and pt_sph_texel_device; no existing struct changes;
                             12: adaptive sampling: converged 8x8 tiles retire from the sample moments
                                (PT_FLAG_ADAPTIVE, pt_adaptive_update, pt_adaptive_status,
                                pt_download_tile_error); no existing struct changes;
                             13: the sample moments and adaptive sampling on screen-tile shares
                                (PT_FLAG_SHARE_MOMENTS, pt_pack_owned_stats, pt_unpack_ranks_stats; pt_adaptive_update
                                and pt_adaptive_status per share); no existing struct changes;
                             13, additive: ray queries with a range, on host arrays and on device memory
                                (pt_trace_closest_range, pt_trace_occluded, pt_trace_closest_device,
                                pt_trace_occluded_device): new symbols only, the version stays;
                             13, additive: geometry updated in place (pt_update_geometry,
                                pt_update_geometry_device, pt_download_node_boxes): new symbols only;
                             13, additive: the integrators as a ray query (pt_radiance_device, pt_radiance) and
                                the frames' camera rays as such rays (pt_camera_rays_device): new symbols only;
                             13, additive: materials updated in place (pt_update_materials,
                                pt_update_materials_device, pt_material_count, pt_download_materials): new
                                symbols only;
                             13, additive: the environment updated in place (pt_update_env, pt_update_env_device,
                                pt_download_env, pt_env_size, PT_ENV_RGBE): new symbols only */

/* error codes */
#define PT_OK 0
#define PT_E_INVALID -1      /* bad argument */
#define PT_E_HIP -2          /* HIP runtime error (see pt_last_error) */
#define PT_E_NOSCENE -3      /* render before pt_upload_scene */
#define PT_E_BADSCENE -4     /* malformed node / triangle arrays */
#define PT_E_NOMEM -5
#define PT_E_IO -6           /* file open / parse failure */
#define PT_E_NODEVICE -7     /* no HIP device / extension missing */

/* integrators (one per reference kernel variant) */
#define PT_LAMBERT_O 0            /* OpenglRayTracing/shaders/pass1.fsh: Lambert, uniform hemisphere, 2 bounces */
#define PT_DISNEY_UNIFORM_D 1     /* DisneyBRDF/shaders/pass1.fsh: aniso Disney, uniform hemisphere, 5 bounces */
#define PT_DISNEY_MIS_SOBOL_IS 2  /* ImportanceSampling_LowDiscrepancySequence/shaders/pass1.fsh: MIS + Sobol, 2 bounces */
#define PT_BASIC_CPU_COMPAT 3     /* BasicRayTracingWithC++/main.cpp: spheres+triangles, RR 0.8, depth 8 */

/* flags */
#define PT_FLAG_NO_CULL 0x1u      /* traverse exactly like pass1.fsh:335-382 (no closest-t culling) */
#define PT_FLAG_CLOSEST_SHADOW 0x2u /* env shadow rays use closest-hit instead of any-hit */
#define PT_FLAG_COUNT_FETCHES 0x4u /* count reference-algorithm fetches (implies NO_CULL, closest shadow) */
#define PT_FLAG_WAVEFRONT 0x8u    /* retired (round 5): the staged wavefront pipeline measured slower than the
                                     regen kernel on every config; pt_create rejects it (PT_E_INVALID) */
#define PT_FLAG_REGEN 0x10u       /* path-regeneration state-machine kernel instead of the megakernel */
#define PT_FLAG_NO_TILE_ORDER 0x20u /* megakernel: hand out tiles in fixed order, not longest-first */
#define PT_FLAG_REFERENCE_TREE 0x40u /* megakernel: traverse only the uploaded tree (not the runtime's own) */
#define PT_FLAG_SERIAL_FRAMES 0x80u /* megakernel: no frames in flight (each frame starts after the previous one ends) */
#define PT_FLAG_NO_BINS 0x100u    /* megakernel: camera rays walk the BVH (no per-tile camera-ray bins) */
#define PT_FLAG_PRIMARY_PASS 0x800u /* camera rays traced by a one-wave-per-tile pass (camera-ray bins) before
                                       the frame kernel instead of inside it: same images; the default for
                                       the large-scene regen kernel (c5 -9 %), slower for the megakernel
                                       on c2-c4. PT_FLAG_NO_BINS turns the pass off */
#define PT_FLAG_MEGAKERNEL 0x400u /* the lock-step megakernel instead of the path-regeneration kernel (4-wide
                                     walk with dynamic ray fetch, camera-ray pass) that large scenes (> 48 MB
                                     of records) and the Lambert integrator on any scene default to */
#define PT_FLAG_HOST_ACCEL 0x200u /* pt_upload_scene builds the runtime's own tree on the host (threaded binned
                                     SAH) instead of on the GPU (pt_build.hip) */
#define PT_FLAG_MOMENTS 0x1000u   /* keep the running means of each sample's luminance and of its square beside
                                     the running mean (pt_download_moments, pt_denoise_var); not with
                                     PT_BASIC_CPU_COMPAT, PT_FLAG_COUNT_FETCHES, PT_FLAG_SERIAL_FRAMES,
                                     tile_world > 1 (unless PT_FLAG_SHARE_MOMENTS) or n_devices > 1 (pt_create:
                                     PT_E_INVALID) */
#define PT_FLAG_ADAPTIVE 0x2000u  /* 8x8 tiles whose pixels have converged stop taking samples (pt_adaptive_update);
                                     needs PT_FLAG_MOMENTS, with every restriction of that flag, and not with
                                     PT_FLAG_NO_BINS (pt_create: PT_E_INVALID). Every frame runs the camera-ray
                                     pass of PT_FLAG_PRIMARY_PASS */
#define PT_FLAG_SHARE_MOMENTS 0x4000u /* PT_FLAG_MOMENTS (and with it PT_FLAG_ADAPTIVE) on a screen-tile share
                                     (tile_world > 1): the moments of the rank's own pixels, gathered with
                                     the running mean (pt_pack_owned_stats, pt_unpack_ranks_stats), and each
                                     rank deciding its own 8x8 tiles. Needs PT_FLAG_MOMENTS, with every other
                                     restriction of that flag, and not with sample_world > 1 (pt_create:
                                     PT_E_INVALID) */

/* in-process multi-GPU (pt_config.n_devices > 1) */
#define PT_MAX_DEVICES 8
#define PT_GATHER_AUTO 0  /* RCCL send/recv when the devices are distinct and RCCL loads, else peer copies */
#define PT_GATHER_COPY 1  /* hipMemcpyPeerAsync of each device's packed tiles to the first device (xGMI) */
#define PT_GATHER_RCCL 2  /* RCCL send/recv group (ncclCommInitAll over device_ids); error if unavailable */

typedef struct pt_config {
  int width;          /* RenderPass::width  (OpenglRayTracing/main.cpp:83), e.g. 1920 */
  int height;         /* RenderPass::height (OpenglRayTracing/main.cpp:84), e.g. 1080 */
  int integrator;     /* PT_LAMBERT_O .. PT_BASIC_CPU_COMPAT */
  int max_bounce;     /* -1 = the reference's default for the integrator */
  int device_id;      /* HIP device ordinal */
  int tile_rank;      /* screen-tile shard owned by this context: tiles t with t % tile_world == tile_rank */
  int tile_world;     /* 1 = whole frame */
  int tile_size;      /* shard tile edge in pixels (0 = 32) */
  uint32_t flags;     /* PT_FLAG_* */
  int basic_samples;  /* PT_BASIC_CPU_COMPAT: SAMPLE (BasicRayTracingWithC++/main.cpp:17), 0 = 128 */
  uint32_t basic_seed;/* PT_BASIC_CPU_COMPAT: seed of the per-pixel counter RNG */
  int sample_rank;    /* sample-parallel rendering: this context draws the RNG/Sobol streams of   */
  int sample_world;   /* samples frameCounter*sample_world + sample_rank (0/1 = the reference's   */
                      /* frameCounter itself); the running-mean weight stays 1/(frameCounter+1)   */
  /* In-process multi-GPU: n_devices >= 2 makes this one context drive
   * device_ids[0..n_devices-1] (device_id is ignored; ids may repeat). Device k renders the
   * 32x32 screen tiles t with t % n_devices == k; every pt_render_frame then gathers the
   * other devices' tiles into device_ids[0]'s accumulation (gather = PT_GATHER_*), so the
   * context's image is bit-identical to a one-device render. tile_world and sample_world
   * must be <= 1 with n_devices >= 2. 0 or 1 = one device (device_id). */
  int n_devices;
  int device_ids[PT_MAX_DEVICES];
  int gather;
  /* ABI 6 */
  int frame_batch;    /* pt_render_frames_async: most frames per launch, at most 32 (0 = automatic:
                         2 x tile_world frames with the Lambert integrator, 4 x tile_world with
                         Disney/MIS, tile_world with Disney/MIS on scenes of more than 48 MB of
                         records -- 12 x / 16 x (32 x for MIS beyond 2 bounces) / 2 x when the hardware queues allow at most 3
                         frames in flight, e.g. HIP's default GPU_MAX_HW_QUEUES = 4) */
  int hw_queues;      /* hardware queues of the process's HIP runtime (GPU_MAX_HW_QUEUES in effect when
                         HIP initialised; bounds the frames in flight); 0 = read GPU_MAX_HW_QUEUES now */
} pt_config;

/* Counters accumulate over every launch since pt_create / pt_reset_stats. */
typedef struct pt_frame_stats {
  uint64_t rays;        /* hitBVH invocations (primary + BRDF + env shadow) */
  uint64_t node_fetch;  /* PT_FLAG_COUNT_FETCHES only: getBVHNode calls (48 B) */
  uint64_t tri_fetch;   /* PT_FLAG_COUNT_FETCHES only: getTriangle calls (72 B) */
  uint64_t mat_fetch;   /* PT_FLAG_COUNT_FETCHES only: getMaterial calls (72 B) */
  uint64_t tex_fetch;   /* PT_FLAG_COUNT_FETCHES only: texel reads (12 B) */
  float kernel_ms;      /* device time of the last render launch (HIP events on its stream) */
  float kernel_ms_total;/* summed device time of the render launches since the reset */
  int launches;         /* render launches since the reset */
  int max_stack;        /* traversal stack bound used (tree depth + 1) */
  int split_items;      /* megakernel: work items the next frame's schedule adds by splitting
                           long-path tiles (0 = one item per tile) */
  int runtime_tree;     /* megakernel: 1 when the last frame traversed the runtime's own tree
                           (results checked against the uploaded one), 0 the uploaded tree */
  int waves_per_simd;   /* megakernel: waves per SIMD the last frame's kernel was compiled for
                           (3 = the large-scene Disney/MIS variant, else its default bound) */
  int devices;          /* devices the context renders on (1, or pt_config.n_devices) */
  int gather;           /* PT_GATHER_COPY / PT_GATHER_RCCL in use (0 with one device) */
  int frames_in_flight; /* megakernel frames that may overlap (1 = serial; >1: kernel_ms of
                           overlapping launches add up to more than the wall time) */
  /* the last pt_upload_scene (kept across pt_reset_stats) */
  float upload_ms;      /* its wall time: host re-layout, copies and the runtime tree build */
  float accel_build_ms; /* wall time of the runtime tree's build (GPU, or host with PT_FLAG_HOST_ACCEL) */
  int accel_device;     /* 1: the runtime tree was built on the GPU, 0: on the host, -1: none */
  int accel_nodes;      /* the runtime tree's nodes (internal + leaves) */
  int accel_depth;      /* and its depth (root = 1) */
  int regen;            /* 1: the last frame ran the path-regeneration kernel (PT_FLAG_REGEN, or a large
                           Disney/MIS scene), 0: the lock-step megakernel */
  /* ABI 6 */
  int64_t frames;       /* frames rendered by the launches since the reset (a batch launch renders
                           several: pt_render_frames_async) */
  int frame_batch;      /* most frames per launch of this context (pt_config.frame_batch, resolved) */
  /* ABI 7 */
  int env_compact;      /* 1: the env is read from its compact texels (RGBE + pdf, 16-bit sample table),
                           which decode to the uploaded floats bit for bit; 2: and the sample table by
                           rows (a row record plus the distinct rows, equal entry by entry); 0: from
                           the float texels */
  int tree4_nodes;      /* 4-wide runtime-tree nodes (0: none) */
} pt_frame_stats;

typedef struct pt_ctx pt_ctx;

/* Device selection, resolution, integrator (replaces glutInit/glewInit/RenderPass
 * setup, OpenglRayTracing/main.cpp:639-644,749-768). */
int pt_create(pt_ctx** out, const pt_config* cfg);
void pt_destroy(pt_ctx* ctx);
const char* pt_last_error(pt_ctx* ctx);  /* ctx may be NULL: last create error */
int pt_device_count(int* n);
int pt_abi_version(void);  /* PT_ABI_VERSION of the loaded library */

/* Upload the encoded scene (replaces the two GL_RGB32F texture buffers,
 * OpenglRayTracing/main.cpp:720-735). tris = nTriangles x 36 f32 exactly as
 * Triangle_encoded (main.cpp:51-60); nodes = nNodes x 12 f32 exactly as
 * BVHNode_encoded (main.cpp:69-73) including the dummy node 0, root at 1. */
int pt_upload_scene(pt_ctx* ctx, const float* tris, int nTriangles, const float* nodes, int nNodes);

/* Geometry updated in place: a deforming or moving object without a new pt_upload_scene (whose host
 * re-layout, copies and caller-side tree build cost many frames). New positions and shading normals for
 * the triangles of the last pt_upload_scene, same count, same order: record i = p1 p2 p3 n1 n2 n3
 * (Triangle_encoded floats 0..17), `stride` floats apart (>= 18; 36 = a whole Triangle_encoded array,
 * whose floats 18..35 are ignored: materials stay). The uploaded tree keeps its topology; every reachable
 * node's box becomes the exact bounds of its triangles (leaves) / of its children (internal nodes), with
 * the reference's min / max (b < a ? b : a, a < b ? b : a), triangles in index order, the left child
 * before the right: the boxes the reference's builders store for that topology (tests/refit_ref.py
 * restates it; an internal node without children keeps its box). The context is then what
 * pt_upload_scene(tris', nodes') would have made it, tris' = the old records with floats 0..17 replaced,
 * nodes' = the old nodes with those boxes: images, query results and counters are bit for bit a fresh
 * upload's. The runtime's own tree is rebuilt on the GPU (a scene whose upload left it on the uploaded
 * tree alone stays there). Everything pt_upload_scene invalidates is invalidated (guides, camera-ray
 * bins, the temporal history, the moments and adaptive state, the measured launch policies): restart
 * at frameCounter 0. pt_frame_stats.upload_ms and accel_* describe the update. Returns when the scene is
 * ready; waits for the frames and queries in flight first. Memory: every uploaded scene keeps its nodes'
 * boxes on the device (32 bytes per node, what the refit writes and pt_download_node_boxes reads), also a
 * scene that never updates or has no runtime tree; the update's own tables (8 bytes per node, 8 per
 * device wide node, 4 per reachable node) and the host form's vertex staging (72 bytes per triangle) are
 * allocated at the first update of a scene.
 * PT_E_NOSCENE before pt_upload_scene and on a PT_BASIC_CPU_COMPAT context; PT_E_INVALID for a NULL
 * pointer, nTriangles != the uploaded count, stride < 18, a PT_FLAG_HOST_ACCEL context (that flag keeps
 * the GPU builder out) and the device form with n_devices > 1 (the host form updates every device).
 * Not part of this: adding, removing or re-sorting triangles (pt_upload_scene), and material changes
 * (pt_update_materials). */
int pt_update_geometry(pt_ctx* ctx, const float* verts, int nTriangles, int stride);
/* the same from device memory of the context's device, read in stream order on the context's stream
 * (pt_set_stream): vertices animated on the GPU need no trip through the host */
int pt_update_geometry_device(pt_ctx* ctx, const void* d_verts, int nTriangles, int stride);
/* diagnostic: the uploaded tree's current boxes, nNodes x 6 f32 (lo, hi) by reference node id; entries
 * of unreachable nodes are unspecified. Synchronous. */
int pt_download_node_boxes(pt_ctx* ctx, float* boxes);

/* Materials updated in place: roughness, base colour, a light's emission, a whole new look, while the
 * geometry stands still -- without a new pt_upload_scene, none of whose triangle re-layout, tree encode,
 * copies, runtime-tree build, camera-ray bins and measured launch policies depends on materials. Record i
 * = the 18 floats at mats + i * stride = Triangle_encoded floats 18..35 of triangle i of the last
 * pt_upload_scene, same count, same order; stride >= 18 (a caller holding a whole Triangle_encoded array
 * passes tris + 18 with stride 36); 4-byte alignment is all that is required. The context is then what
 * pt_upload_scene(tris', nodes) would have made it, tris' = the current records with floats 18..35
 * replaced: images of every integrator through every launch form, ray counts, PT_FLAG_COUNT_FETCHES
 * counters, pt_radiance* and guide buffers are bit for bit a fresh upload's. So is the material table:
 * distinct keys -- compared as 18 uint32, never as floats: +0 and -0 differ, two NaNs of the same bits
 * are one key -- numbered by their first appearance in triangle order, whatever order the GPU's atomics
 * land in (pt_materials.hip). Two floats are unspecified: a table entry is stored as floats 16..35 of
 * its first triangle; no kernel reads the first two, pt_update_geometry leaves them stale, this update
 * zeroes them, and pt_download_materials does not return them.
 * Invalidated: the guides (their albedo is stale: pt_denoise* and pt_temporal_resolve return
 * PT_E_INVALID until the next pt_render_guides), the temporal history, the moments and adaptive state:
 * restart at frameCounter 0. Kept: the uploaded tree, the runtime tree and its 4-wide collapse, the
 * traversal stack bound, the camera-ray bins and the measured launch policies -- no tree build runs.
 * (The guides are invalidated by their own flag: the scene version that the guides and the camera-ray
 * bins both compare against is not bumped, since the bins hold geometry only.) pt_frame_stats.upload_ms
 * describes the update; accel_*, max_stack, tree4_nodes and runtime_tree are unchanged. Returns when the
 * scene is ready; waits for the frames and queries in flight first.
 * Memory, allocated at a scene's first material update and freed with the scene (a scene that never
 * updates pays nothing): a material table with room for one material per triangle (80 bytes per
 * triangle, in place of the upload's) and the update's own tables (12 bytes per triangle, 4 bytes per
 * slot of a probe table of the next power of two >= 2 x nTriangles slots: 8 to 16 bytes per triangle,
 * and the scan's scratch); the host form also stages its records (72 bytes per triangle).
 * PT_E_NOSCENE before pt_upload_scene and on a PT_BASIC_CPU_COMPAT context; PT_E_INVALID for a NULL
 * pointer, nTriangles != the uploaded count, stride < 18 and the device form with n_devices > 1 (the
 * host form updates every device). PT_FLAG_HOST_ACCEL contexts are allowed: nothing is built. A failed
 * call leaves the context usable. */
int pt_update_materials(pt_ctx* ctx, const float* mats, int nTriangles, int stride);
/* the same from device memory of the context's device, read in stream order on the context's stream
 * (pt_set_stream): materials animated on the GPU need no trip through the host */
int pt_update_materials_device(pt_ctx* ctx, const void* d_mats, int nTriangles, int stride);
/* the number of distinct materials of the scene (the table's entries) */
int pt_material_count(pt_ctx* ctx, int* nMats);
/* diagnostic: the material table -- min(nMats, maxMats) entries of 18 f32 (Triangle_encoded floats
 * 18..35) in table order -- and every triangle's id (nTriangles i32); either may be NULL, not both.
 * Also on a scene that was never updated: the upload's table. Synchronous. */
int pt_download_materials(pt_ctx* ctx, float* table, int maxMats, int* ids);

/* Upload the HDR environment (replaces hdrMap/hdrCache textures,
 * ImportanceSampling_LowDiscrepancySequence/main.cpp:843-853). hdr = w x h x 3
 * f32, row 0 = first scanline; cache = calculateHdrCache output (nullable: the
 * library computes it). hdrResolution := w. hdr == NULL clears the env (black). */
int pt_upload_env(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache);

/* A new environment in place: after the call the context is what pt_upload_env(ctx, hdr', w, h, cache)
 * would have made it, where hdr' is hdr -- or, with PT_ENV_RGBE, hdr with every texel rounded to the RGBE
 * texel a Radiance file would hold (include/pt_rgbe.h: negative values, -0 and NaN become 0, values above
 * 255 * 2^119 that value, a texel whose largest channel would be stored below 1e-32f black), so that a map computed in
 * floats is kept in the compact forms a decoded file's is. cache == NULL: the library's table, computed on
 * the device from hdr'; a caller's table is used as given, also with PT_ENV_RGBE. Images of every
 * integrator through every launch form, ray counts, PT_FLAG_COUNT_FETCHES counters, pt_radiance*,
 * pt_frame_stats.env_compact and what pt_download_env returns are bit for bit a fresh upload's.
 * hdr == NULL clears the environment, as pt_upload_env(NULL) does.
 * The work runs on the GPU on the context's stream: the texels are packed, the library's table computed,
 * the compact forms, Env::light and the table by rows built (pt_envupdate.hip), and three ints come back
 * in the call's one host synchronisation -- texels and table compact, rows in row form, distinct rows --
 * from which the forms that serve are chosen. It waits for the frames and queries in flight first and
 * returns when the environment is ready.
 * Invalidated, as pt_upload_env does: the temporal history, the moments and adaptive state: restart at
 * frameCounter 0. Kept: the scene, both trees, the camera-ray bins and the guides (they hold no
 * environment data), and the measured launch policies while w, h and the resulting env_compact are what
 * they were before the call (otherwise they are measured again, as after pt_upload_env).
 * Memory: the buffers belong to the map's size. The first update of a w x h map allocates them -- 24 bytes
 * per texel for the float texels and table; with w, h <= 65535 another 12 for the compact forms, 2 for the
 * rows' y's, about 8 for Env::light, and 4 (h + 65536) + 8 (w + h + 2) bytes of row and angle tables,
 * whether or not that map is compact -- and every later update of the same size reuses them and allocates
 * and frees nothing; Env::trig is computed once per size. A map that is not compact leaves the compact
 * buffers allocated and unused. At its first use each kind of update adds what it needs: without a caller's
 * table 24 bytes per texel for the library's table and its scratch (12 more with PT_ENV_RGBE); the host
 * form 12 bytes per texel of staging, 24 with a table. Another size, pt_upload_env or pt_destroy frees
 * them all; on another size the previous environment stays in place until the new one is complete.
 * PT_E_INVALID for a NULL context, w <= 0 or h <= 0 with a map, a map whose 3 * w * h, (w + 1)(h + 1) or
 * table scratch count does not fit an int, unknown flag bits and a PT_BASIC_CPU_COMPAT context; PT_E_NOMEM
 * when the float texels, the library table's scratch or the staging cannot be allocated. Every other
 * table (the compact forms, trig, light, rows) falls back to the form before it instead. A failed call
 * leaves the previous environment in place and the context usable. PT_UPDATE_TIMES (environment
 * variable): the device time of each step on stderr. */
#define PT_ENV_RGBE 0x1u /* round every texel to the RGBE texel a Radiance file would hold, first */
int pt_update_env(pt_ctx* ctx, const float* hdr, int w, int h, const float* cache, uint32_t flags);
/* the same from device memory of the context's device (w*h*3 f32, row 0 = first scanline; d_cache
 * w*h*3 f32 as pt_hdr_cache writes it, or NULL), read in stream order on the context's stream
 * (pt_set_stream): a sky computed or edited on the GPU needs no trip through the host. PT_E_INVALID with
 * n_devices > 1 (the host form updates every device). */
int pt_update_env_device(pt_ctx* ctx, const void* d_hdr, int w, int h, const void* d_cache, uint32_t flags);
/* diagnostic, synchronous: the environment as the kernels read it -- texels w*h*4 f32 (r, g, b, pdf) and
 * the sample table w*h*2 f32 (x, y); either may be NULL, not both. form 0: the float texels and table.
 * form 1: the same values decoded from the compact texels and the compact table by the frame kernels'
 * decoders; PT_E_INVALID when env_compact < 1. form 2: the table read through the row form by the frame
 * kernels' lookup; PT_E_INVALID when env_compact < 2 or texels != NULL (the rows hold no texels). Forms 1
 * and 2 equal form 0 bit for bit. Also after pt_upload_env. PT_E_INVALID without an environment. */
int pt_download_env(pt_ctx* ctx, int form, float* texels, float* table);
int pt_env_size(pt_ctx* ctx, int* w, int* h); /* the environment's size; 0, 0 without one */

/* PT_BASIC_CPU_COMPAT shape list (the vector<Shape*> of BasicRayTracingWithC++/main.cpp:306-353):
 * n x 24 f64 records (layout in pt_scene.h; the reference's Material rates and sphere radius
 * are doubles, its vec3 fields floats). */
int pt_upload_shapes(pt_ctx* ctx, const double* shapes, int n);

/* PT_BASIC_CPU_COMPAT: the reference's `double* image` (BasicRayTracingWithC++/main.cpp:356,
 * summed by :427-429; row 0 = top), width x height x 3 f64 host buffer. The f32 accumulation
 * (pt_download_accum) holds the same sums rounded to float. */
int pt_download_basic_image(pt_ctx* ctx, double* rgb);
/* PT_BASIC_CPU_COMPAT checkpoint restore: the double image (as pt_download_basic_image wrote it);
 * the next frame adds its sample to it, bit for bit as if the frames had not been interrupted.
 * (pt_upload_accum on a BASIC context restores from the f32 sums: the double image is set to
 * them, widened.) */
int pt_upload_basic_image(pt_ctx* ctx, const double* rgb);

/* PT_BASIC_CPU_COMPAT: replay a recorded random stream instead of the per-pixel counter RNG,
 * so a frame consumes exactly the random numbers the reference's serial run consumed
 * (its one global std::mt19937 read by randf(), main.cpp:208-214). stream = n doubles in
 * draw order; offsets[(k * height + i) * width + j] = the stream position at which sample k
 * of pixel (row i from the top, column j) starts (n_offsets = samples * width * height; a
 * sample's draws end where the next one's start). A pixel sample that would read past its
 * end gets 0.5 and is counted (pt_basic_replay_overruns). stream == NULL switches back to
 * the counter RNG. Frame frameCounter renders sample k = frameCounter. */
int pt_set_basic_stream(pt_ctx* ctx, const double* stream, int64_t n, const int64_t* offsets, int64_t n_offsets);
int pt_basic_replay_overruns(pt_ctx* ctx, int64_t* count);

/* calculateHdrCache (ImportanceSampling_LowDiscrepancySequence/main.cpp:555-652)
 * computed on this context's GPU; output as pt_hdr_cache (w*h*3 f32: sample x,
 * sample y, pdf), bit-identical to it. pt_upload_env with cache = NULL uses it. */
int pt_hdr_cache_device(pt_ctx* ctx, const float* hdr, int w, int h, float* cache_out);

/* One display() (OpenglRayTracing/main.cpp:558-603): 1 spp per owned pixel and
 * the running-mean update of the device-resident accumulation (pass1.fsh:868-871);
 * frameCounter = 0 resets the mean (mix weight 1). eye[3]; cameraRotate[16]
 * column-major = inverse(lookAt(eye, 0, up)) (main.cpp:570-573). accum_rgba
 * (nullable) receives width x height x 4 f32 after the frame. For
 * PT_BASIC_CPU_COMPAT frameCounter is the sample index k and accum is the sum
 * buffer `image` (BasicRayTracingWithC++/main.cpp:356-431). */
int pt_render_frame(pt_ctx* ctx, const float eye[3], const float cameraRotate[16],
                    uint32_t frameCounter, float* accum_rgba);
/* Same without synchronising or downloading. */
int pt_render_frame_async(pt_ctx* ctx, const float eye[3], const float cameraRotate[16],
                          uint32_t frameCounter);
/* nFrames display() calls of one camera: frames frameCounter .. frameCounter + nFrames - 1, each
 * 1 spp per owned pixel with its own running-mean update (bit for bit nFrames calls of
 * pt_render_frame_async). Consecutive frames are rendered side by side in one launch (up to
 * pt_config.frame_batch; while the tree / split policies are being measured, one each) and
 * their running-mean updates applied together, pixel by pixel in frame order; the accumulation
 * holds the last frame's mean when the call's work completes (a frame in between is not
 * materialised in it). Without synchronising. */
int pt_render_frames_async(pt_ctx* ctx, const float eye[3], const float cameraRotate[16],
                           uint32_t frameCounter, int nFrames);

/* The GPU binned-SAH builder (pt_build.hip), exposed as a scene
 * builder in the reference's node encoding -- the role of buildBVH / buildBVHwithSAH
 * (OpenglRayTracing/main.cpp:376-551), with pt_scene.h PT_BVH_BINNED_SAH's split rule.
 * tris = nTriangles x 36 f32 (Triangle_encoded; only p1..p3 are read). Writes
 * *nNodes_out nodes (12 f32 each: dummy node 0, root 1, leaves of <= leafSize
 * triangles whose ranges index the built order) to nodes_out when they fit in
 * max_nodes (else PT_E_INVALID, *nNodes_out still set), and order_out[i] = the input
 * index of the triangle at built position i (nTriangles ints). */
int pt_build_bvh_device(pt_ctx* ctx, const float* tris, int nTriangles, int leafSize, float* nodes_out,
                        int max_nodes, int* nNodes_out, int* order_out);

/* The origin domain. Every result is the reference traversal's whichever tree is walked, for every ray
 * origin and every eye. The runtime's own tree is walked only from origins in its domain:
 *     max(|o.x|, |o.y|, |o.z|) <= 32 x the scene scale,
 * the scene scale being the largest coordinate magnitude of the uploaded (or last updated) triangles' vertices
 * (csrc/pt_scene_prep.cpp prepareAccel derives the 32 from the widening of that tree's boxes). Outside it,
 * and for an origin with a NaN or an infinite coordinate, the results are the same ones, found through the
 * uploaded tree alone: per ray in pt_trace_closest, the ranged and occlusion queries, pt_radiance* and
 * pt_radiance_mean* (a path's bounce rays start on the scene and are in the domain), per launch for the eye
 * of pt_render_frame* and pt_render_guides -- pt_frame_stats.runtime_tree then reads 0 for that frame, and
 * what the launch policy measured with such an eye is measured again at the next restart. Only the time
 * differs: the uploaded tree's walk is the slower one on most scenes. */

/* Batch hitBVH (pass1.fsh:335-382; BVH/main.cpp:571 debug-ray query). rays =
 * n x 6 f32 (origin, direction); miss -> t = 2147483648.f, tri = -1. */
int pt_trace_closest(pt_ctx* ctx, const float* rays, int n, float* t_out, int* tri_out);

/* Ray queries with a range, on host arrays or on device memory: the closest hit below a bound, and the
 * occlusion test (what a ray-casting library offers beside "closest": ambient occlusion, visibility
 * between points, light baking on the uploaded scene). Both are stated against pt_trace_closest. With
 * (t*, tri*) its result for ray k and b = tmax[k] (tmax NULL: every t* passes):
 *   ranged closest: (t*, tri*) if tri* >= 0 && t* < b, else the miss values (2147483648.f, -1)
 *   occluded:       1          if tri* >= 0 && t* < b, else 0
 * The comparison is strict (b == t* is a miss), a NaN b is a miss, and so is b <= 0.0005f (hitTriangle's
 * own lower bound, pass1.fsh:251-301). The walk starts its closest-hit bound at b, so a short range costs
 * a short walk, and the occlusion test ends at the first hit it may report. The context's flags apply as
 * they do to pt_trace_closest (PT_FLAG_NO_CULL, PT_FLAG_REFERENCE_TREE, PT_FLAG_COUNT_FETCHES; the
 * default is the runtime's tree with the reference check). pt_frame_stats is not touched. With
 * n_devices > 1 the queries run on device_ids[0]. PT_E_NOSCENE before pt_upload_scene; PT_E_INVALID for
 * n < 0 or a NULL required pointer with n > 0; n == 0 is PT_OK and reads and writes nothing.
 *
 * The host forms are synchronous. Unlike pt_trace_closest they do not wait for the frames in flight:
 * the queries have a traversal stack overflow area of their own and may overlap frames. */
int pt_trace_closest_range(pt_ctx* ctx, const float* rays /* n x 6 f32 */, const float* tmax /* n f32, NULL: no bound */,
                           int n, float* t_out, int* tri_out);
int pt_trace_occluded(pt_ctx* ctx, const float* rays, const float* tmax, int n, uint8_t* occ_out /* n u8: 0 / 1 */);
/* The device forms: every pointer is device memory of the context's device. Asynchronous, in stream
 * order on the context's stream (pt_set_stream), after any pt_upload_scene issued before them; no host
 * synchronisation, and no allocation after the first query of a scene (the overflow area is sized at
 * first use and again after an upload that deepens the trees). Work another stream queued on d_rays or
 * d_tmax is not ordered before the query, nor the query before another stream's reads of its results:
 * set that stream with pt_set_stream, or synchronise first (as with pt_display_*). */
int pt_trace_closest_device(pt_ctx* ctx, const void* d_rays /* n x 6 f32 */, const void* d_tmax /* n f32 or NULL */, int n,
                            void* d_t /* n f32 */, void* d_tri /* n i32 */);
int pt_trace_occluded_device(pt_ctx* ctx, const void* d_rays, const void* d_tmax, int n, void* d_occ /* n u8: 0 / 1 */);

/* Radiance along caller-supplied rays: one sample of the context's integrator (PT_LAMBERT_O, PT_DISNEY_UNIFORM_D
 * or PT_DISNEY_MIS_SOBOL_IS, with the context's max_bounce) along each ray, for cameras the frame kernels do
 * not have (panorama, fisheye, thin lens), radiance probes, light-map bakes and a caller's own secondary
 * rays. For ray k = (o, d) with id (px, py) = d_ids[k] and sample index s = sampleIndex:
 *   - d_ids NULL: the id is (k & 4095, k >> 12), which gives every k < 2^23 its own seed
 *     (px * 1973 + py * 9277 is injective for px < 9277, py < 1973);
 *   - d is used as given: the caller normalises it, and t is in units of |d|;
 *   - (t, tri) is pt_trace_closest's result for the ray. A miss: out = (SampleHdr of the environment
 *     along d, 2147483648.f), black without an environment. A hit: the hit record the frame kernels
 *     compute for a camera hit, then the integrator;
 *   - the path's RNG state is that of seed (px * 1973 + py * 9277 + s * 26699) | 1 (pass1.fsh main) after
 *     two discarded rand() draws: what a frame's pixel (px, py) of sample s holds once its jittered
 *     camera ray exists. For PT_DISNEY_MIS_SOBOL_IS the Sobol index is s and the Cranley-Patterson shift
 *     that of (px, py);
 *   - out.rgb = Le(first hit) + Li, the sum a frame adds to its running mean; out.w = t.
 * The contract: if ray k is bit for bit the ray pt_camera_rays_device writes for (px, py, s) of some
 * camera and image size, out[k].rgb is bit for bit the sample a frame with sample index s (frameCounter *
 * sample_world + sample_rank) gives that pixel -- whatever k, n, the other rays and this context's own
 * width and height are.
 * One sample per call: fold several calls with the running-mean weights 1 / (i + 1), or let
 * pt_radiance_mean_device below take and fold many samples in one call. The context's flags
 * apply as they do to the ray queries (PT_FLAG_NO_CULL, PT_FLAG_REFERENCE_TREE, PT_FLAG_COUNT_FETCHES; the
 * default is the runtime's tree with the reference check). pt_frame_stats is not touched. With
 * n_devices > 1 the call runs on device_ids[0]. PT_E_NOSCENE before pt_upload_scene and on a
 * PT_BASIC_CPU_COMPAT context; PT_E_INVALID for n < 0 or a NULL required pointer (rays, out) with n > 0;
 * n == 0 is PT_OK and reads and writes nothing.
 * The device form is asynchronous, in stream order on the context's stream as the device ray queries
 * are (after any pt_upload_scene or pt_update_geometry issued before it), allocates nothing in the steady
 * state and may overlap frames in flight; it shares the ray queries' stack overflow area, so it takes its
 * turn among them. d_out must be 16-byte aligned. The host form stages in and out and is synchronous. */
int pt_radiance_device(pt_ctx* ctx, const void* d_rays /* n x 6 f32 */, const void* d_ids /* n x 2 i32 or NULL */,
                       int n, uint32_t sampleIndex, void* d_out /* n x 4 f32: r, g, b, t */);
int pt_radiance(pt_ctx* ctx, const float* rays, const int* ids, int n, uint32_t sampleIndex, float* out);
/* Many samples per call, folded on the GPU: the radiance query's counterpart of pt_render_frames_async and
 * PT_FLAG_MOMENTS. For ray k and j = 0 .. nSamples-1, with s = firstSample + j:
 *   - c_j is pt_radiance_device's out[k].rgb for sample index s along ray rays[k], bit for bit -- or, with
 *     PT_RADIANCE_RAYS_PER_SAMPLE, along ray rays[j * n + k]: the array is then nSamples x n x 6 f32, for a
 *     caller who jitters per sample;
 *   - the fold, one IEEE f32 operation per step (no fused multiply-add), is the frames' running-mean update:
 *       w = 1.0f / (float)(s + 1u);  a = mixf(a, c_j, w) per channel, mixf(x, y, w) = x * (1.0f - w) + y * w;
 *       l = (0.3f r + 0.6f g) + 0.1f b of c_j;  m1 = mixf(m1, l, w);  m2 = mixf(m2, l * l, w);
 *   - firstSample == 0 starts from a = 0 and m = 0: d_mean and d_moments are not read, whatever they hold.
 *     Otherwise a is read from d_mean[k].rgb and m from d_moments[k], so a picture goes on across calls
 *     exactly as frames do across launches;
 *   - d_mean[k] = (a, t of the last sample's ray, 2147483648.f on a miss); d_moments[k] = (m1, m2), not
 *     touched when d_moments is NULL.
 * Without PT_RADIANCE_RAYS_PER_SAMPLE the ray's closest hit is searched once for all its samples, and a
 * ray that leaves the scene folds its one sky colour nSamples times.
 * The consequence: with per-sample rays equal to pt_camera_rays_device's of samples 0 .. N-1 and ids (px, py),
 * firstSample 0 and nSamples N, d_mean.rgb is bit for bit the accumulation of pt_render_frames_async(.., 0, N)
 * and d_moments bit for bit a PT_FLAG_MOMENTS context's plane.
 * Everything else as pt_radiance_device: the default ids, the context's flags, device_ids[0], pt_frame_stats
 * untouched, stream order on the context's stream, its turn among the queries (one overflow area), frames in
 * flight may overlap it, no allocation in the steady state; d_mean must be 16-byte aligned, d_moments 8-byte.
 * PT_E_INVALID for nSamples < 1, firstSample + nSamples > 2^32 - 1 (the weight's s + 1u must not wrap),
 * unknown flag bits, n < 0, or a NULL rays or mean with n > 0; PT_E_NOSCENE before pt_upload_scene and on a
 * PT_BASIC_CPU_COMPAT context; n == 0 is PT_OK and reads and writes nothing.
 * The host form stages rays, ids, mean and moments in and mean and moments out, and is synchronous. */
#define PT_RADIANCE_RAYS_PER_SAMPLE 0x1u /* rays is nSamples x n x 6 f32: sample j's ray k at rays[j * n + k] */
int pt_radiance_mean_device(pt_ctx* ctx, const void* d_rays, const void* d_ids /* n x 2 i32 or NULL */, int n,
                            uint32_t firstSample, int nSamples, uint32_t flags,
                            void* d_mean /* n x 4 f32: r, g, b, t */, void* d_moments /* n x 2 f32 or NULL */);
int pt_radiance_mean(pt_ctx* ctx, const float* rays, const int* ids, int n, uint32_t firstSample, int nSamples,
                     uint32_t flags, float* mean, float* moments);
/* The frame kernels' camera rays of sample sampleIndex, jitter included, for every pixel of the context's
 * width x height: ray py * width + px = (eye, the pixel's jittered direction), id = (px, py). Asynchronous on
 * the context's stream. PT_E_INVALID on a PT_BASIC_CPU_COMPAT context or for a NULL d_rays. */
int pt_camera_rays_device(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t sampleIndex,
                          void* d_rays /* width*height x 6 f32 */, void* d_ids /* width*height x 2 i32, nullable */);

/* Accumulation buffer access (lastFrame texture, main.cpp:763-764). */
int pt_download_accum(pt_ctx* ctx, float* accum_rgba);   /* host or device memory, width*height*4 f32 */
int pt_upload_accum(pt_ctx* ctx, const float* accum_rgba);
int pt_clear_accum(pt_ctx* ctx);
int pt_accum_device_ptr(pt_ctx* ctx, void** dptr); /* width*height*4 f32, device memory */

/* pass3.fsh tonemap c / (1 + (0.3r+0.6g+0.1b)/limit) of the accumulation,
 * optional gamma (pass3.fsh:14-24 keeps it commented out: gamma <= 0). rgb_out
 * = width x height x 3 f32 host buffer. */
int pt_tonemap(pt_ctx* ctx, float limit, float gamma, float* rgb_out);

/* Multi-process tile exchange (one process per GPU, pt_config.tile_rank/tile_world):
 * pack this rank's owned pixels into a contiguous device buffer (count =
 * pt_owned_pixel_count slots of 3 f32: r, g, b -- a rendered pixel's alpha is
 * always 1, and unpack writes 1), and unpack another rank's packed pixels into this
 * context's accumulation. Pointers are device memory; the caller moves the
 * packed buffers (RCCL gather over xGMI). Not for n_devices > 1 contexts, which
 * gather inside pt_render_frame. */
int pt_owned_pixel_count(pt_ctx* ctx, int rank, int world, int64_t* count);
int pt_pack_owned(pt_ctx* ctx, void* dpacked);
int pt_unpack_rank(pt_ctx* ctx, int rank, int world, const void* dpacked);
/* pt_unpack_rank of ranks 1..world-1 in one launch (dpacked[k] = rank k's packed buffer, [0] unused,
 * a NULL entry is skipped; world <= 16): rank 0's reassembly after a gather of the running means. */
int pt_unpack_ranks(pt_ctx* ctx, int world, const void* const* dpacked);

/* The displayed frame (pass3.fsh:14-24 drawn into the 8-bit GLUT_RGBA window,
 * ImportanceSampling_LowDiscrepancySequence/main.cpp:706,747): tonemap (and gamma > 0)
 * of the accumulation, stored as round(clamp(x, 0, 1) * 255) per channel, alpha 255.
 * A screen-tile split presents every frame from 3 bytes per pixel instead of the
 * accumulation's 12: each rank packs its owned pixels' display values
 * (pt_display_pack: pt_owned_pixel_count slots of 3 u8, packed order as pt_pack_owned),
 * the caller moves them to rank 0 (RCCL gather over xGMI), and rank 0 writes its own
 * tiles (pt_display_own) and the other ranks' (pt_display_unpack: dpacked[k] = rank k's
 * packed buffer for k = 1..world-1, world <= 16, one launch) into one width x height
 * RGBA8 device image. With tile_world 1, pt_display_own writes every pixel. All on the
 * context's current stream, after the frames rendered so far; device pointers (work
 * another stream queued on those buffers is not ordered before it: set that stream
 * with pt_set_stream, or synchronise it first). */
int pt_display_pack(pt_ctx* ctx, float limit, float gamma, void* dpacked);
int pt_display_own(pt_ctx* ctx, float limit, float gamma, void* dimage);
int pt_display_unpack(pt_ctx* ctx, int world, const void* const* dpacked, void* dimage);

/* Guide buffers and the denoised display. The interactive frame is 1 spp per display(): for the
 * first seconds after a camera move the running mean is noisy. pt_render_guides traces the camera
 * ray through every pixel centre once per camera, and pt_denoise filters the running mean with an
 * edge-avoiding a-trous wavelet (Dammertz et al. 2010) steered by those guides; pt_display_denoised
 * presents the result through the 8-bit display path. The accumulation is only read: progressive
 * frames continue from it unchanged. The filter is an exact sequence of IEEE f32 operations
 * (tests/denoise_ref.py restates it; the GPU output equals it bit for bit). */
typedef struct pt_denoise_params {
  int   passes;       /* 1..8; pass i uses tap stride 2^i */
  float sigma_c;      /* colour term, on tone-mapped colour, halved every pass; <= 0: off */
  float sigma_z;      /* plane-distance term, relative to the centre's hit distance; <= 0: off */
  float sigma_a;      /* albedo term; <= 0: off */
  int   normal_log2;  /* normal weight max(0, Np.Nq)^(2^normal_log2), 0..10; -1: off */
  float limit;        /* the tonemap limit used inside the colour term (pass3: 1.5) */
} pt_denoise_params;
#define PT_DENOISE_PARAMS_SIZE 24 /* sizeof(pt_denoise_params), asserted by the library (pt_denoise_params_size) */

void pt_denoise_defaults(pt_denoise_params* prm);  /* 5, 2.0, 0.02, 0.2, 6, 1.5 */
int pt_denoise_params_size(void);                  /* sizeof(pt_denoise_params) of the loaded library */

/* The camera's first hit of every pixel of the whole frame (a tile_world > 1 context's non-owned
 * pixels included): the frame kernels' camera ray with the jitter terms 0 (the pixel centre), pt_trace_closest's
 * hit search (reference tie rules), then the integrators' hit record. Three float4 planes,
 * width x height each, row 0 = the bottom row like the accumulation:
 *   pos_t   = (P.x, P.y, P.z, t)
 *   nrm_tri = (N.x, N.y, N.z, int bits of the uploaded triangle index), N the facing-flipped
 *             shading normal the integrators use
 *   albedo  = (baseColor.rgb, 1)
 * a miss: (0, 0, 0, 2147483648.f), (0, 0, 0, bits(-1)), (0, 0, 0, 0). Context-owned device memory,
 * valid until the next pt_render_guides, pt_upload_scene or pt_destroy. Asynchronous, on the
 * context's stream; pt_frame_stats is not touched (no rays, launches or frames counted). With
 * n_devices > 1 they are rendered on device_ids[0]. Not for PT_BASIC_CPU_COMPAT. */
int pt_render_guides(pt_ctx* ctx, const float eye[3], const float cameraRotate[16]);
/* each width*height*4 f32, nullable, host or device memory; synchronous */
int pt_download_guides(pt_ctx* ctx, float* pos_t, float* nrm_tri, float* albedo);
int pt_guides_device_ptr(pt_ctx* ctx, void** pos_t, void** nrm_tri, void** albedo);  /* each nullable */

/* The a-trous filter of the accumulation, steered by the last pt_render_guides (PT_E_INVALID
 * before one, or after pt_upload_scene invalidated it). prm NULL = pt_denoise_defaults. For pass
 * i = 0 .. passes-1 (stride s = 2^i, colour sigma sigma_c 2^-i, c the pass's input, tm(c) =
 * pt_tonemap's expression with gamma off and limit prm->limit): a miss pixel is copied; a hit pixel
 * p sums the 25 taps q = p + s (dx, dy) that are inside the image and hits, with
 *   k = H[|dx|] H[|dy|], H = {0.375, 0.25, 0.0625};  n = max(0, Np.Nq) squared normal_log2 times;
 *   a = |Np.(Pq - Pp)| / (sigma_z t_p) + |tm(cq) - tm(cp)|^2 / sigma_c_i^2 + |Aq - Ap|^2 / sigma_a^2;
 *   w = (k n) exp(-a);   out.rgb = sum(cq w) / sum(w) (cp.rgb when the sum is not > 0), out.w = cp.w.
 * The last pass writes d_out_rgba (width*height*4 f32 device memory), or with NULL a
 * context-owned buffer (pt_denoised_device_ptr). Asynchronous, on the context's stream, after
 * the frames rendered so far. */
int pt_denoise(pt_ctx* ctx, const pt_denoise_params* prm, void* d_out_rgba);
/* pt_denoise reading d_in_rgba (width*height*4 f32 device memory, e.g. pt_resolved_device_ptr)
 * instead of the accumulation; NULL = the accumulation (pt_denoise is this call with NULL). The
 * input's .w is carried through. d_in_rgba is only read; it must not be d_out_rgba or the
 * context's own denoised buffer (pt_denoised_device_ptr): PT_E_INVALID. */
int pt_denoise_from(pt_ctx* ctx, const pt_denoise_params* prm, const void* d_in_rgba, void* d_out_rgba);
int pt_denoised_device_ptr(pt_ctx* ctx, void** dptr);
/* the last pt_denoise's image, width*height*4 f32 into host or device memory; synchronous */
int pt_download_denoised(pt_ctx* ctx, float* rgba);
/* pt_display_own's tonemap and 8-bit store of the last pt_denoise's image (every pixel, whatever
 * tile_world is), into a width x height RGBA8 device image. PT_E_INVALID before any pt_denoise. */
int pt_display_denoised(pt_ctx* ctx, float limit, float gamma, void* dimage);

/* The running mean reprojected across camera moves. Every caller of pt_render_frame restarts at
 * frameCounter = 0 when the camera moves, so during a drag each presented picture is a 1-spp image
 * and what the previous cameras accumulated is lost. The scene is static: the first-hit position P
 * that pt_render_guides holds for a pixel projects straight into the previous camera, with no new
 * ray. pt_temporal_resolve fetches the previous camera's resolved image there (bilinear, each tap
 * tested against the centre's plane and normal) and blends it with the running mean of the new
 * camera, weighted by sample count; pt_temporal_commit makes the resolved image and the current
 * guides the history of the next camera. The accumulation is only read and pt_frame_stats is not
 * touched. The step is an exact sequence of IEEE f32 operations (tests/temporal_ref.py restates it;
 * the GPU output equals it bit for bit).
 *
 * The display() loop:  if (cameraMoved) { pt_temporal_commit; pt_render_guides; frameCounter = 0; }
 *                      pt_render_frame; pt_temporal_resolve(frames = frameCounter + 1);
 *                      pt_denoise_from(resolved); pt_display_denoised.
 *
 * Limits: the history holds the radiance the previous cameras saw, so view-dependent (glossy)
 * shading lags behind the camera: lower max_history there. */
typedef struct pt_temporal_params {
  float sigma_z;      /* a history tap is accepted when |Np.(Pq - Pp)| <= sigma_z * t_p; >= 0 */
  float normal_cos;   /* ... and Np.Nq >= normal_cos, in [-1, 1] */
  float max_history;  /* cap of the reprojected sample count, >= 1 */
} pt_temporal_params;
#define PT_TEMPORAL_PARAMS_SIZE 12 /* sizeof(pt_temporal_params), asserted by the library (pt_temporal_params_size) */

void pt_temporal_defaults(pt_temporal_params* prm);  /* 0.02, 0.9, 32 */
int pt_temporal_params_size(void);                   /* sizeof(pt_temporal_params) of the loaded library */

/* One resolve of the whole frame (whatever tile_world is: rank 0 calls it after the unpack), steered
 * by the last pt_render_guides, which must be of the camera the accumulation was rendered with
 * (PT_E_INVALID before one or after pt_upload_scene invalidated it, as pt_denoise). prm NULL =
 * pt_temporal_defaults. frames = the frames in the accumulation, frameCounter + 1 (0: PT_E_INVALID).
 * With c the accumulation, kf = (float)frames, E' / M' the history camera's eye and cameraRotate,
 * c0 = M'[0..2], c1 = M'[4..6], c2 = M'[8..10], dot(a, b) = (ax bx + ay by) + az bz, per pixel p:
 *   out = (c.rgb, kf)
 *   with a history, for a hit pixel:
 *     v = Pp - E';  a = dot(c0, v);  b = dot(c1, v);  cz = dot(c2, v);  s = -1.5 / cz
 *     fx = (a s + 1) (0.5 W) - 0.5;  fy = (b s + 1) (0.5 H) - 0.5
 *     ok = cz < 0 && -1 < fx < W && -1 < fy < H;  (ix, iy) = floor(fx, fy);  (tx, ty) = the fractions
 *     the taps q = (ix + i, iy + j), j = 0, 1 outer, i = 0, 1 inner, bilinear weight wt: valid when q is
 *     inside the image, a hit of the history, hist[q].w > 0, |Np.(Pq - Pp)| <= sigma_z t_p and
 *     Np.Nq >= normal_cos;  wv = valid ? wt : 0;  sw += wv;  sum += hist[q].rgb wv;  sn += hist[q].w wv
 *     ok && sw > 0:  hc = sum / sw;  n = min(sn / sw, max_history);  wgt = kf / (n + kf);
 *                    out = (hc (1 - wgt) + c.rgb wgt, n + kf)
 * A miss pixel shows the environment texel directly and takes no history. Without a history (before
 * the first commit, after pt_temporal_reset, pt_upload_scene or pt_upload_env) out is the
 * accumulation's rgb, bit for bit, with count kf. The width x height float4 plane goes to
 * d_out_rgba (device memory), or with NULL to a context-owned buffer (pt_resolved_device_ptr).
 * Resolving again without a commit recomputes from the same history. Asynchronous, on the context's
 * stream, after the frames rendered so far. With n_devices > 1 on device_ids[0]. Not for
 * PT_BASIC_CPU_COMPAT. */
int pt_temporal_resolve(pt_ctx* ctx, const pt_temporal_params* prm, uint32_t frames, void* d_out_rgba);
/* The last resolved image, the current guides' pos_t and nrm_tri and the camera they were rendered
 * with become the history. Nothing is copied: the context keeps two resolved planes and two sets of
 * pos_t / nrm_tri; every later pt_render_guides writes the set that is not the history (so
 * pt_guides_device_ptr may alternate), and the current guides stay valid and readable until then.
 * PT_E_INVALID when no pt_temporal_resolve has run since the last commit, reset or
 * pt_render_guides, or when the last resolve went to a caller's buffer (d_out_rgba != NULL): the
 * library keeps no reference to memory the caller may overwrite -- resolve with NULL to commit. */
int pt_temporal_commit(pt_ctx* ctx);
int pt_temporal_reset(pt_ctx* ctx);  /* drops the history (as pt_upload_scene and pt_upload_env do) */
/* the last pt_temporal_resolve's image (PT_E_INVALID before one) */
int pt_resolved_device_ptr(pt_ctx* ctx, void** dptr);
int pt_download_resolved(pt_ctx* ctx, float* rgba);  /* host or device memory, width*height*4 f32; synchronous */
/* pt_display_denoised of the last pt_temporal_resolve's image */
int pt_display_resolved(pt_ctx* ctx, float limit, float gamma, void* dimage);

/* Per-pixel sample moments. pt_denoise filters a converged image exactly as hard as a 1-spp one: nothing
 * above knows how noisy a pixel still is. A PT_FLAG_MOMENTS context keeps, beside the running mean of
 * the colour, the running means m1 and m2 of l and l l, l = (0.3 r + 0.6 g) + 0.1 b of each frame's
 * sample colour (pt_tonemap's luminance), in a width x height plane of (m1, m2) pairs, row 0 = the
 * bottom row, zero at creation. They take the accumulation's own weight: for frame frameCounter + f of a
 * launch, w = 1 / (float)(frameCounter + f + 1), m1 = m1 (1 - w) + l w, m2 = m2 (1 - w) + (l l) w, each
 * operation one IEEE f32 operation (tests/variance_ref.py restates it; the GPU equals it bit for bit),
 * so frameCounter = 0 restarts them as it restarts the mean. The accumulation itself is bit for bit a
 * plain context's. With sample_world > 1 the moments are of this context's own samples.
 *
 * The context counts the frames the moments hold: a launch with frameCounter == 0 sets the count to
 * its frames, a launch whose frameCounter equals the count adds its frames, any other frameCounter
 * sets it to 0 (not valid), and so do pt_upload_accum, pt_clear_accum (which also zeroes the plane),
 * pt_upload_scene, pt_upload_env, pt_unpack_rank and pt_unpack_ranks (the last two not on a
 * PT_FLAG_SHARE_MOMENTS context, below). */
int pt_moments_frames(pt_ctx* ctx, uint32_t* frames);  /* 0: not valid, or no PT_FLAG_MOMENTS */
/* width*height*2 f32 into host or device memory, after the frames rendered so far; synchronous.
 * PT_E_INVALID without PT_FLAG_MOMENTS. */
int pt_download_moments(pt_ctx* ctx, float* m);
int pt_moments_device_ptr(pt_ctx* ctx, void** dptr);   /* PT_E_INVALID without PT_FLAG_MOMENTS */

/* The variance-guided a-trous filter (Schied et al. 2017, "Spatiotemporal Variance-Guided Filtering",
 * its spatial part): pt_denoise's filter with the colour term replaced by a luminance term in units
 * of each pixel's estimated standard deviation, so that it filters a noisy pixel hard and a converged
 * one hardly at all. The filter is an exact sequence of IEEE f32 operations (correctly rounded sqrt,
 * pt_fmath.h's exp; tests/variance_ref.py restates it; the GPU output equals it bit for bit). */
typedef struct pt_denoise_var_params {
  int   passes;        /* 1..8; pass i uses tap stride 2^i */
  float sigma_l;       /* luminance term, in standard deviations, the same in every pass; <= 0: off */
  float sigma_z;       /* as pt_denoise_params */
  float sigma_a;       /* as pt_denoise_params */
  int   normal_log2;   /* as pt_denoise_params */
  float limit;         /* as pt_denoise_params */
  int   min_temporal;  /* the moments are used once they hold this many frames; >= 2 */
} pt_denoise_var_params;
#define PT_DENOISE_VAR_PARAMS_SIZE 28 /* sizeof(pt_denoise_var_params), asserted by the library */

void pt_denoise_var_defaults(pt_denoise_var_params* prm);  /* 5, 4.0, 0.02, 0.2, 6, 1.5, 8 */
int pt_denoise_var_params_size(void);                      /* sizeof(pt_denoise_var_params) of the loaded library */

/* Filters d_in_rgba (width*height*4 f32 device memory, e.g. pt_resolved_device_ptr; NULL = the
 * accumulation; the aliasing rule of pt_denoise_from) into d_out_rgba, or with NULL into the context's
 * denoised buffer: pt_denoised_device_ptr, pt_download_denoised and pt_display_denoised serve both
 * filters. Needs valid guides, with pt_denoise's checks and error codes. prm NULL =
 * pt_denoise_var_defaults. lum(c) = (0.3 r + 0.6 g) + 0.1 b, tm as in pt_denoise, max(x, y) = x > y ? x : y,
 * kf = (float)pt_moments_frames.
 * Step A, the variance v of the input's tone-mapped luminance, 0 at a miss pixel:
 *   kf >= min_temporal:  L = lum(c_p);  q = 1 + L / limit;  gd = 1 / (q q) (the tonemap's slope);
 *                        n_p = max(c_p.w, kf) (the accumulation's .w is 1, a resolved image's its sample
 *                        count);  v = (max(m2 - m1 m1, 0) / n_p) (gd gd)
 *   else, or without PT_FLAG_MOMENTS (rank 0 of a plain tile split; during a drag): over the 7 x 7 window
 *                        around p (dy outer, dx inner, -3..3) the pixels q inside the image that are hits:
 *                        l_q = lum(tm(c_q));  s1 += l_q;  s2 += l_q l_q;  cnt += 1;
 *                        v = max(s2 / cnt - (s1 / cnt) (s1 / cnt), 0)
 * Step B, pass i = 0 .. passes-1 (stride s = 2^i, inputs c and v, l = lum(tm(c))): a miss pixel copies c
 * and v; a hit pixel p takes
 *   vt_p = sum(v_q g) / sum(g) over its 3 x 3 neighbours q (dy outer, dx inner, -1..1) inside the image
 *          that are hits, g = G[|dx|] G[|dy|], G = {0.5, 0.25};   lden = sigma_l sqrt(vt_p) + 1e-6
 *   and the 25 taps q = p + s (dx, dy) of pt_denoise, with its k and n:
 *   a = |Np.(Pq - Pp)| / (sigma_z t_p) + |l_q - l_p| / lden + |Aq - Ap|^2 / sigma_a^2;   w = (k n) exp(-a);
 *   out.rgb = sum(c_q w) / sum(w),  v_out = sum(v_q (w w)) / (sum(w) sum(w))  (c_p.rgb and v_p when
 *   sum(w) is not > 0),  out.w = c_p.w.
 * Asynchronous, on the context's stream, after the frames rendered so far. */
int pt_denoise_var(pt_ctx* ctx, const pt_denoise_var_params* prm, const void* d_in_rgba, void* d_out_rgba);
/* Test hook: step A's plane of the last pt_denoise_var, width*height f32 into host or device memory;
 * synchronous. PT_E_INVALID before one. */
int pt_download_variance(pt_ctx* ctx, float* v);

/* Adaptive sampling. Every frame above spends one sample on every pixel for as long as the caller keeps
 * rendering. A PT_FLAG_ADAPTIVE context (a PT_FLAG_MOMENTS context, too) can stop: pt_adaptive_update
 * looks at every 8x8 tile of the image -- tile (tx, ty) is entry ty * tilesX + tx, tilesX = (width + 7) / 8,
 * row 0 at the bottom like the accumulation -- and retires those whose pixels have all converged. A
 * retired tile costs nothing from then on: the camera-ray pass writes it an empty mask, so no frame
 * kernel claims it, no ray of it is traced or counted, and the running-mean update leaves its pixels
 * alone. Retirement is permanent until the running mean restarts, which keeps everything exact: an
 * active pixel has taken every frame so far, so its weight 1 / (frameCounter + f + 1) is still the right
 * one and its accumulation and moments are bit for bit a PT_FLAG_MOMENTS context's; a retired pixel
 * keeps, bit for bit, the accumulation and moments it had at the update that retired its tile.
 *
 * The decision, with kf = (float)pt_moments_frames, thr2 = threshold * threshold, for every tile T that
 * is not retired, over its pixels inside the image, each operation one IEEE f32 operation
 * (tests/adaptive_ref.py restates it; the GPU equals it bit for bit):
 *   L = (0.3 r + 0.6 g) + 0.1 b of the accumulation;  q = 1 + L / limit;  gd = 1 / (q q)
 *   d = m2 - m1 m1;  d = d > 0 ? d : 0;  v = (d / kf) (gd gd)       (pt_denoise_var's step A with n_p = kf,
 *                                                                    without guides: sky pixels count too)
 *   err2[T] = the largest v (e = v > e ? v : e from 0: a NaN never wins)
 *   frames >= min_frames and err2[T] <= thr2:  retired_at[T] = frames
 * A tile retired earlier keeps its err2 and retired_at. Both planes are zero at creation and are
 * cleared, with every tile active again, by a launch with frameCounter == 0 and by everything that
 * invalidates the moments (pt_upload_accum, pt_clear_accum, pt_upload_scene, pt_upload_env). A gap in
 * frameCounter (moments not valid) leaves the retired tiles retired until such a restart; updates fail
 * meanwhile.
 *
 * The display() loop:
 *   pt_render_frame_async(ctx, eye, rot, frameCounter);
 *   if (frameCounter % N == N - 1) {
 *     pt_adaptive_update(ctx, &prm);
 *     pt_adaptive_status(ctx, &st);
 *     if (st.retired == st.tiles) stop;       (the picture is done)
 *   }
 *   frameCounter++;
 * Not part of this: device groups (excluded with PT_FLAG_MOMENTS), decisions finer than a tile,
 * un-retiring, and retirement carried across camera moves. Screen-tile shares: PT_FLAG_SHARE_MOMENTS
 * below. */
typedef struct pt_adaptive_params {
  float threshold;   /* a pixel has converged when the standard error of the mean of its tone-mapped
                        luminance is <= threshold; > 0 and finite */
  float limit;       /* the tonemap limit of that luminance (pass3: 1.5); > 0 */
  int   min_frames;  /* no tile retires before the moments hold this many frames; >= 2 */
} pt_adaptive_params;
#define PT_ADAPTIVE_PARAMS_SIZE 12 /* sizeof(pt_adaptive_params), asserted by the library */

void pt_adaptive_defaults(pt_adaptive_params* prm);  /* 1 / 255.f, 1.5, 16 */
int pt_adaptive_params_size(void);                   /* sizeof(pt_adaptive_params) of the loaded library */

typedef struct pt_adaptive_state {
  int tiles;            /* 8x8 tiles of the image: tilesX * tilesY (a PT_FLAG_SHARE_MOMENTS share: those it owns) */
  int retired;          /* of them retired */
  uint32_t frames;      /* pt_moments_frames at the last update (0: none since the restart) */
  float max_err2;       /* the largest err2 over the tiles still active (0 when none is) */
} pt_adaptive_state;
#define PT_ADAPTIVE_STATE_SIZE 16 /* sizeof(pt_adaptive_state), asserted by the library */
int pt_adaptive_state_size(void);                    /* sizeof(pt_adaptive_state) of the loaded library */

/* One decision over every active tile. prm NULL = pt_adaptive_defaults. PT_E_INVALID without
 * PT_FLAG_ADAPTIVE, with bad parameters, while pt_moments_frames is 0, and when the context's launches
 * cannot run the camera-ray pass (no runtime tree for the camera-ray bins: nothing could retire).
 * Asynchronous, on the context's stream, after the frames rendered so far; frames rendered after it see
 * its result, every frame of one launch the same one. */
int pt_adaptive_update(pt_ctx* ctx, const pt_adaptive_params* prm);
/* Synchronous. PT_E_INVALID without PT_FLAG_ADAPTIVE. */
int pt_adaptive_status(pt_ctx* ctx, pt_adaptive_state* st);
/* The tile planes, `tiles` entries each, either may be NULL, host or device memory: err2 as the last
 * update that looked at the tile left it, retired_at the frame count at which the tile retired (0:
 * active). Synchronous. PT_E_INVALID without PT_FLAG_ADAPTIVE. */
int pt_download_tile_error(pt_ctx* ctx, float* err2, uint32_t* retired_at);

/* The sample moments and adaptive sampling on a screen-tile split. A shard tile's edge is a multiple of
 * 8, so every 8x8 tile of the image belongs to exactly one rank: each rank can keep the moments of its
 * own pixels and decide its own tiles, and nothing of that needs another rank. A PT_FLAG_SHARE_MOMENTS
 * context (PT_FLAG_MOMENTS with tile_world > 1, PT_FLAG_ADAPTIVE too) does:
 *  - The moments plane is still width x height. After a launch it holds this rank's values at the pixels
 *    it owns -- bit for bit what a one-context PT_FLAG_MOMENTS render holds there (the same update of the
 *    same floats) -- and everywhere else what was last unpacked (zero at creation). pt_moments_frames
 *    counts this rank's own frames, by the rule above.
 *  - pt_unpack_rank, pt_unpack_ranks and pt_unpack_ranks_stats do not invalidate the moments and leave the
 *    tile planes alone: they write other ranks' pixels only. (On a context without the flag they invalidate
 *    as before.) pt_upload_accum, pt_clear_accum, pt_upload_scene, pt_upload_env, a gap in frameCounter and
 *    the restart at frameCounter == 0 keep their effect.
 *  - pt_adaptive_update decides the 8x8 tiles this rank owns and writes only their entries of the two
 *    planes, which stay whole-image planes (pt_download_tile_error: 0 at every other rank's entries). The
 *    ranks' planes have disjoint support: the image's planes are their element-wise sums.
 *  - pt_adaptive_status counts the tiles this rank owns (0 for a rank past the last shard tile, whose
 *    updates succeed and do nothing); the image's status is the sum of the ranks' tiles and retired and the
 *    largest of their max_err2.
 *  - pt_denoise_var and pt_temporal_resolve on rank 0 after pt_unpack_ranks_stats see a whole moments
 *    plane, and kf = pt_moments_frames selects step A's moments branch.
 *
 * pt_pack_owned_stats: pt_pack_owned with the moments -- pt_owned_pixel_count slots of 5 f32 (r, g, b,
 * m1, m2), the packed order of pt_pack_owned, a slot outside the image zeros. One launch on the context's
 * stream, after the frames rendered so far. pt_unpack_ranks_stats: pt_unpack_ranks of such buffers
 * (dpacked[k] = rank k's, [0] unused, a NULL entry is skipped; world <= 16), one launch: the accumulation
 * (r, g, b, 1) and the moments (m1, m2) of every other rank's pixels. The caller guarantees that every
 * rank rendered the same frames: rank 0's pt_moments_frames is then the count of the whole plane. Both
 * PT_E_INVALID without PT_FLAG_SHARE_MOMENTS and for n_devices > 1 contexts.
 *
 * The display() loop of N ranks, one batch of frames per round (rank r of N):
 *   pt_render_frames_async(ctx, eye, rot, frameCounter, n);  frameCounter += n;
 *   pt_pack_owned_stats(ctx, send);
 *   gather send to rank 0's recv[r] (RCCL over xGMI);
 *   rank 0:  pt_unpack_ranks_stats(ctx, N, recv);            (may run on a communication stream,
 *                                                             pt_set_stream, while the next batch renders)
 *   every K rounds:
 *     pt_adaptive_update(ctx, &prm);  pt_adaptive_status(ctx, &st);
 *     all-reduce: tiles = sum st.tiles, retired = sum st.retired, max_err2 = max st.max_err2;
 *     if (retired == tiles) every rank stops;                 (the picture is done)
 *   rank 0:  pt_render_guides;  pt_denoise_var;  pt_display_denoised.
 * Not part of this: device groups, sample_world > 1, re-dealing tiles among the ranks as they retire. */
#define PT_PACK_STATS_F 5 /* f32 per slot of pt_pack_owned_stats */
int pt_pack_owned_stats(pt_ctx* ctx, void* dpacked);
int pt_unpack_ranks_stats(pt_ctx* ctx, int world, const void* const* dpacked);

/* Stream interop: render on the caller's HIP stream (e.g. torch's current
 * stream). NULL restores the context's own stream. */
int pt_set_stream(pt_ctx* ctx, void* hip_stream);
int pt_synchronize(pt_ctx* ctx);
int pt_get_stats(pt_ctx* ctx, pt_frame_stats* stats);   /* synchronises the stream */
int pt_reset_stats(pt_ctx* ctx);

/* Diagnostics: evaluate one include/pt_fmath.h function (0 sin, 1 cos, 2 atan2(x,y),
 * 3 asin, 4 log, 5 exp, 6 pow(x,y), 7 ptm_atan2f_fast(x,y), 8 ptm_asinf_fast, 9 / 10 the sine / the
 * cosine that ptm_sincosf returns) over n inputs on the host CPU or on the
 * context's GPU; the two must agree bit for bit. */
int pt_fmath_host(int fn, const float* x, const float* y, int n, float* out);
int pt_fmath_device(pt_ctx* ctx, int fn, const float* x, const float* y, int n, float* out);
/* Diagnostics: the sky texel y * W + x that the frame kernels' fast decision (pt_device.h sphTexel)
 * and its correctly rounded fallback (sphTexelExact) give for each of n directions (dirs: n x 3 f32),
 * evaluated on the directions exactly as given (not normalised), for a W x H map (W * H < 2^31).
 * Needs no env upload. The two outputs must be equal for every direction. */
int pt_sph_texel_device(pt_ctx* ctx, int W, int H, const float* dirs, int n, int* texel, int* texel_exact);

#ifdef __cplusplus
}
#endif
#endif /* PT_ABI_H */
