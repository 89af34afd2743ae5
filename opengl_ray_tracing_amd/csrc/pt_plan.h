// pt_plan.h -- the launch policy of the frame path (pt_context.cpp createOne, pt_scene_upload.cpp uploadScene, pt_runtime.cpp renderOne):
// which kernel, tree, camera-ray pass, bins and table form a launch uses, how many frames a launch
// takes and how many launches are in flight. Pure functions of the context and the configuration:
// no HIP call, no environment, nothing written to the context (tests/native/plan_table.cpp calls
// them on contexts filled by hand, without a device). Internal: not installed.
#pragma once
#include <algorithm>
#include <cstddef>

#include "pt_runtime.h"

// The tuning knobs of the policy (tools/tune.py and tools/ab_*.sh pass them with -D).
// 32: c2's 1/8 share in the 20-frame bench window at 4 hardware queues 0.0417 -> 0.0351 ms per
// frame (its 20 frames one launch instead of 16 + 4), 1/4 share 0.0593 -> 0.0569, c4 0.2736 -> 0.2701
#ifndef PT_MAX_BATCH
#define PT_MAX_BATCH 32
#endif
static constexpr int MAX_BATCH = PT_MAX_BATCH;  // most frames per launch (pt_render_frames_async)
#ifndef PT_BATCH_LAMBERT
#define PT_BATCH_LAMBERT 12  // c2, 20 frames: 8 + 8 + 4 -> 12 + 8, 0.1789-0.1802 -> 0.1707-0.1729 ms (10: 0.1949); 200 frames equal
#endif
#ifndef PT_BATCH_MIS
#define PT_BATCH_MIS 16
#endif
#ifndef PT_BATCH_MIS_MK
// MIS beyond its shader's 2 bounces renders on the megakernel (c4): 32 frames per launch, c4 0.2599
// -> 0.2327 ms over 20 frames (one launch instead of 16 + 4), 0.2389 -> 0.2303 over 100; the MIS
// regen kernel (c3) keeps 16 (24 / 32: 0.1107 -> 0.1122 / 0.1148)
#define PT_BATCH_MIS_MK 32
#endif
#ifndef PT_TILE_GROUP
#define PT_TILE_GROUP 1  // tiles ordered by cost in groups of this many consecutive tiles (1 measured best)
#endif
// A launch's share of the machine while others are in flight, in % of its equal share (gridFor)
#ifndef PT_GRID_PCT
#define PT_GRID_PCT 125  // round 5, final kernels: c4 0.2571 -> 0.2463 ms at 150 -> 125, its 1/8 share 0.0721 -> 0.0688, c2's 0.0332 -> 0.0325; 175: c2 +3 %
#endif
#ifndef PT_GRID_PCT_WIDE
#define PT_GRID_PCT_WIDE 150  // large scenes (c5: two frames per launch, ~8 ms launches): 4.44 ms at 125
#endif

// the scene's records on the device (uploadScene keeps it in pt_ctx::sceneBytes)
static inline size_t sceneBytes(int nTri, int nDevNodes) {
  return (size_t)nTri * (PAIR_F4 * 16 + 64 + HIT_F4 * 16) + (size_t)nDevNodes * 64;
}

// the scene's records outgrow the L2s by far (pt_kernels.h PT_WIDE_SCENE_MB)
static inline bool largeScene(const pt_ctx* ctx) { return ctx->sceneBytes > ((size_t)PT_WIDE_SCENE_MB << 20); }

// the env sample table by rows for a launch of a lock-step kernel (the megakernel, the radiance query)
// when the table outgrows an XCD's L2 share, 4 MB: c4's frame kernel 216 -> 147 MB DRAM-side per frame,
// time unchanged (0.2914 / 0.2927 ms); never for the regen kernel (regen), whose walks the extra
// dependent load costs more than their misses (c5 4.20 -> 4.31 ms, c3 0.1083 -> 0.111)
static inline bool rowTable(const pt_ctx* ctx, bool regen) {
  return !regen && (size_t)ctx->hdrW * ctx->hdrH * sizeof(uint32_t) > ((size_t)4 << 20);
}

static inline int defaultBounce(int integ) {
  switch (integ) {
    case PT_LAMBERT_O: return 2;           // O:385
    case PT_DISNEY_UNIFORM_D: return 5;    // D:502
    case PT_DISNEY_MIS_SOBOL_IS: return 2; // IS:861
    default: return 8;                     // BasicRayTracingWithC++/main.cpp:254
  }
}

static inline int maxBounce(const pt_config& c) { return c.max_bounce >= 0 ? c.max_bounce : defaultBounce(c.integrator); }

// the default megakernel and the regen kernel pipeline their frames (not BASIC, the fetch
// counter or PT_FLAG_SERIAL_FRAMES)
static inline bool pipelines(const pt_config& c) {
  return c.integrator != PT_BASIC_CPU_COMPAT && !(c.flags & (PT_FLAG_COUNT_FETCHES | PT_FLAG_SERIAL_FRAMES));
}

// The Disney/MIS integrators on large scenes: by default the regen kernel's (WIDE_REGEN_WAVES), whose
// walks are memory-latency bound and whose long paths leave a lock-step wave's lanes idle. Such
// scenes run 4 frames in flight (uploadScene).
static inline bool wideScene(const pt_ctx* ctx) {
  const pt_config& c = ctx->cfg;
  return !(c.flags & (PT_FLAG_COUNT_FETCHES | PT_FLAG_NO_CULL)) && c.integrator != 0 && largeScene(ctx);
}

// Frames in flight of a pipelined context (createOne; PT_PIPE_DEPTH overrides it there, and uploadScene
// caps it at 4 on wideScene scenes). A process has the hardware queues its HIP runtime was initialised
// with: streams beyond them share queues and serialise, so the slot streams, the context's own stream
// and the caller's (torch's) must fit.
// Whole Lambert frames (the regen kernel on every scene): 6 in flight. c2's bench line (20 frames
// from an idle GPU) 0.254-0.257 ms per frame at 6 vs 0.259-0.277 at 8 and 0.259 at 4, 100 frames
// 0.232 either way; the MIS megakernel keeps 8 (c4 0.366 at 8 vs 0.373-0.397 at 6, 0.41 at 4),
// and so do screen-tile shares (c2's 1/8 share 0.061 at 8 vs 0.074 at 6)
static inline int pipeDepthFor(const pt_config& c, int regenWide, int hwQueues) {
  int depth = std::min(PT_PIPE, std::max(2, hwQueues - 2));
  if (c.integrator == 0 && regenWide != 0 && c.tile_world <= 1) depth = std::min(depth, 6);
  return depth;
}

// Frames per launch of pt_render_frames_async: pt_config.frame_batch, else whole images' work per
// launch in multiples of tile_world frames, at most MAX_BATCH:
//  * 2 x for the Lambert regen kernel -- one image's is enough to fill the machine, the second
//    halves the launches and running-mean updates per frame: c2 0.244 -> 0.231 ms per frame at
//    N = 1, c2's 1/8 share 0.0354 -> 0.0344 (profiles/r4); 3 and 4 measured no better;
//  * 4 x for the megakernel (Disney/MIS on small scenes), whose longest-first launches end in their
//    longest tiles: c4 at N = 1 0.2566 -> 0.2531 ms per frame over 200 frames and 0.3288 -> 0.2860
//    over 20 from an idle GPU, N = 2 0.139 -> 0.131, N = 4 / 8 equal (profiles/r4/batch_c4/);
//  * 1 x on large Disney/MIS scenes, whose frames are long already (c5 5.66 ms at 1, 5.86 at 2).
// With few hardware queues (GPU_MAX_HW_QUEUES 4, HIP's default and the GPU box's: 2 frames in flight)
// a launch takes more frames, so that about as much work is in flight: Lambert 8 x, Disney/MIS 16 x,
// large scenes 2 x (round 5, 4 queues, the driver's 20-frame bench window from an idle GPU: c2 at
// 2 / 4 / 6 / 8 / 12 / 16 frames per launch 0.218 / 0.196 / 0.187 / 0.184 / 0.178 / 0.184 ms per
// frame; c4 at 4 / 8 / 16 0.342 / 0.302 / 0.271; c5 at 1 / 2 4.59 / 4.34; c2's shares at 20 frames,
// N = 2 / 4 / 8, at 2 x N 0.116 / 0.066 / 0.041 and 4 x N 0.107 / 0.060 / 0.041 ms).
static inline int batchFor(const pt_ctx* ctx, bool wideScene) {
  const pt_config& c = ctx->cfg;
  if (c.frame_batch > 0) return std::min(c.frame_batch, MAX_BATCH);
  const bool fewQueues = ctx->pipeDepth <= 3;
  const int mis = c.integrator == 2 && maxBounce(c) > 2 ? PT_BATCH_MIS_MK : PT_BATCH_MIS;
  const int m = wideScene ? (fewQueues ? 2 : 1) : c.integrator == 0 ? (fewQueues ? PT_BATCH_LAMBERT : 2) : (fewQueues ? mis : 4);
  return std::max(1, std::min(m * std::max(1, c.tile_world), MAX_BATCH));
}

// What a launch uses, decided before anything is enqueued (renderOne; the tree and the split policy
// are probePolicy's, the launch shape the occupancy queries')
struct FramePlan {
  bool count;      // the fetch-counting megakernel (PT_FLAG_COUNT_FETCHES)
  bool cull;
  bool wideScene;
  bool regenAll;   // the regen kernel with the large-scene path on scenes of any size (pt_ctx::regenWide)
  bool oneCall;    // a single frame with nothing else in flight: the megakernel
  bool regen;      // the path-regeneration kernel, else the lock-step megakernel
  bool wide;       // the more-waves variant of either kernel
  bool walk4;      // ... walking the 4-wide runtime tree
  bool pass;       // the camera-ray pass ahead of the frame kernel
  bool bins;       // camera rays through the camera-ray bins
  bool rowTable;   // the env sample table by rows
  int envNt;       // RenderParams::env.nt
  bool ordered;    // longest-tiles-first: each band's tiles in the order of the previous frame's cost
  bool piped;      // the launch runs on a slot of the pipeline (a colour buffer, a running-mean update launch)
};

// The eye of a frame or guide launch against the origin domain of the runtime tree in place (pt_kernels.h
// originInDomain; pt_scene_prep.cpp prepareAccel derives it). A launch whose eye is outside runs without
// that tree -- SceneView::fast 0, no 4-wide walk, no camera-ray bins (their winners are checked by the
// same margin argument) -- so every ray of it takes the reference-order walk of the uploaded tree, and
// pt_frame_stats.runtime_tree reads 0 for it. The paths' bounce rays start on the scene, always in domain,
// but one launch walks one tree.
static inline bool eyeInDomain(const pt_ctx* ctx, const float eye[3]) {
  return originInDomain(eye[0], eye[1], eye[2], ctx->originLimit);
}

// a launch of this context is one of the frames in flight
static inline bool pipedFrames(const pt_ctx* ctx) { return ctx->pipe && !(ctx->cfg.flags & PT_FLAG_COUNT_FETCHES); }

// solo: the launch is issued while no other is in flight, on the caller's stream; want: the frames
// the caller asked for; eyeIn: the launch's eye is in the runtime tree's origin domain (eyeInDomain)
static inline FramePlan planFrame(const pt_ctx* ctx, bool solo, int want, bool eyeIn = true) {
  const pt_config& c = ctx->cfg;
  FramePlan f;
  f.count = (c.flags & PT_FLAG_COUNT_FETCHES) != 0;
  f.cull = !f.count && !(c.flags & PT_FLAG_NO_CULL);
  // default: the lock-step persistent megakernel (also the fetch-counting
  // variant); the path-regeneration kernel on request, and by default for the
  // Disney/MIS integrators on large scenes (wideScene above)
  f.wideScene = wideScene(ctx);
  // ... and the MIS integrator at its shader's own 2 bounces (IS:861): c3 at 4 hardware queues 0.1443 ->
  // 0.1331 ms per frame on the regen kernel (round 5); deeper MIS paths keep the megakernel (c4, 8
  // bounces: 0.270 vs 0.370)
  f.regenAll = !f.count && f.cull &&
               (ctx->regenWide > 0 ||
                (ctx->regenWide < 0 && (c.integrator == 0 || (c.integrator == 2 && maxBounce(c) <= 2))));
  f.piped = pipedFrames(ctx);
  // The frame kernel. A single frame issued while nothing else is in flight -- a synchronous
  // display() call (pt_render_frame), SURVEY 8(d)'s per-call time -- runs on the lock-step megakernel,
  // which splits its long tiles and orders its work longest first, where the regen kernel's launch
  // ends in its waves' last paths at falling lane counts: per call c3 0.585 -> 0.373 ms, c2 0.449 ->
  // 0.439 (c4 is on the megakernel already: 0.78; its regen kernel 1.32). Streams of frames keep
  // the regen kernel (c2's batches 0.17 ms per frame). PT_FLAG_REGEN pins the regen kernel.
  f.oneCall = f.piped && solo && want == 1 && !largeScene(ctx) && ctx->regenWide <= 0;
  f.regen = !f.count && ((c.flags & PT_FLAG_REGEN) ||
                         ((f.wideScene || (f.regenAll && !f.oneCall)) && !(c.flags & PT_FLAG_MEGAKERNEL)));
  // the more-waves variant of either kernel (the regen kernel's with its 4-wide walk, dynamic ray
  // fetch and camera-ray pass; on small trees with the whole tree in LDS)
  f.wide = f.wideScene || (f.regen && f.regenAll);
  f.walk4 = f.wide && ctx->fast4Ready && eyeIn && !(c.flags & PT_FLAG_REFERENCE_TREE);
  f.rowTable = rowTable(ctx, f.regen);
  f.envNt = largeScene(ctx) ? 1 : 0;
  const int group = std::max(1, PT_TILE_GROUP);
  f.ordered = !f.regen && !f.count && !(c.flags & PT_FLAG_NO_TILE_ORDER) &&
              (ctx->perQueue + group - 1) / group <= REORDER_MAX && ctx->numItems < (1 << 22);
  // The camera-ray pass (primaryKernel) traces the camera rays ahead of the frame kernel: on
  // request, and by default for the large-scene regen kernel (c5 7.52 -> 6.86 ms), whose lanes
  // then start from the camera ray's hit; the megakernel is faster with its camera rays inside
  // (c2 0.372 vs 0.383 ms with the pass). Adaptive sampling retires tiles in the pass: every kernel
  // of a PT_FLAG_ADAPTIVE context runs behind it
  f.pass = (c.flags & (PT_FLAG_PRIMARY_PASS | PT_FLAG_ADAPTIVE)) || (f.regen && f.wide);
  // camera-ray bins need the reference facts refReachable checks a bin's winner against
  f.bins = PT_BINS && !f.count && ctx->fastReady && eyeIn && !(c.flags & PT_FLAG_NO_BINS) && (!f.regen || f.pass);
  return f;
}
