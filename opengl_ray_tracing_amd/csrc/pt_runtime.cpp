// pt_runtime.cpp -- the frame path of the C-ABI in include/pt_abi.h: launch timing, the tree / split
// policy probe, the slots of the frames in flight, one launch step by step (renderOne), and
// pt_render_frame[s][_async]. Its helpers are static: an 8-way share of c2 runs at about 0.04 ms per
// frame and is bounded by the host's launch chain, so nothing here calls into another file that it
// could call in this one. (What the launches decide without a HIP call is pt_plan.h.) The file keeps
// the name it had when it held the whole host runtime, so the history of the most measured code stays
// with it; the context's life is pt_context.cpp, the other subjects are listed in pt_runtime.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_kernels.h"
#include "pt_plan.h"
#include "pt_runtime.h"

using namespace pt;

static_assert(PT_PIPE >= 1 && PT_PIPE <= PIPE, "PT_PIPE: 1..MAX_SLOTS");
static_assert(PIPE * NUM_QUEUES * CTL_LINE_INTS * 4 <= (int)CTL_STATS, "queue counters of every slot fit the control block");

// One family of per-frame buffers -- the colour buffers, the slots' camera-ray results or their
// live-item lists -- with room in bufs[idx] for the launch's `frames` frames. Every buffer of the n a
// pipelined context uses (n = 0: unpiped, bufs[idx] alone) is allocated at the first launch that uses
// any, so no later launch -- a timed one -- waits for an allocation (c2's 1/8 share: a 19 us hipMalloc
// before the sixth launch's first kernel). A buffer too small is freed after wait() -- its last
// reader -- and allocated again (each buffer grows once, to batchCap). bytes(cap): of cap frames.
template <class T, class Bytes, class Wait>
static int frameBuffer(pt_ctx* ctx, T** bufs, int* caps, int n, int idx, int frames, int cap, Bytes bytes, Wait wait) {
  auto alloc = [&](int k) -> int {
    CK(hipMalloc(&bufs[k], bytes(cap)));
    caps[k] = cap;
    return PT_OK;
  };
  for (int k = 0; k < n; k++)
    if (!bufs[k])
      if (int rc = alloc(k)) return rc;
  if (caps[idx] >= frames) return PT_OK;
  if (bufs[idx]) {
    CK(wait());
    dfree(bufs[idx]);
  }
  return alloc(idx);
}

// Fold the oldest unfolded launch's device time into the totals (and into its
// probe slot). blocking = false returns false instead of waiting for it.
static bool foldOne(pt_ctx* ctx, bool blocking) {
  if (ctx->folded >= ctx->issued) return false;
  const int k = (int)(ctx->folded % EV_RING);
  hipEvent_t b = ctx->ev[2 * k], e = ctx->ev[2 * k + 1];
  if (blocking) (void)hipEventSynchronize(e);
  else if (hipEventQuery(e) != hipSuccess) return false;
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, b, e) != hipSuccess) ms = 0.0f;
  ctx->msTotal += ms;
  ctx->msLast = ms;
  const int slot = ctx->evProbe[k];
  if (slot >= 0 && ctx->evGen[k] == ctx->probeGen) {
    ctx->probeMs[slot] += ms;
    ctx->probeN[slot]++;
  }
  ctx->folded++;
  return true;
}

// fold every launch up to launch number `upto` (inclusive), waiting for them
static void foldUpTo(pt_ctx* ctx, long long upto) {
  while (ctx->folded <= upto && foldOne(ctx, true)) {
  }
}

// ... and every launch issued so far (the stats and their reset)
void foldLaunches(pt_ctx* ctx) {
  while (foldOne(ctx, true)) {
  }
}

// begin/end events for the next launch (launch number ctx->issued)
static int launchEvents(pt_ctx* ctx, hipEvent_t* b, hipEvent_t* e) {
  while (foldOne(ctx, false)) {
  }
  if (ctx->issued - ctx->folded >= EV_RING) foldOne(ctx, true);
  const int k = (int)(ctx->issued % EV_RING);
  for (int j = 2 * k; j < 2 * k + 2; j++)
    if (!ctx->ev[j]) CK(hipEventCreate(&ctx->ev[j]));
  *b = ctx->ev[2 * k];
  *e = ctx->ev[2 * k + 1];
  return PT_OK;
}

// the launch whose events launchEvents handed out has been enqueued (it renders `frames` frames)
static void commitLaunch(pt_ctx* ctx, int frames = 1) {
  ctx->frames += frames;
  const int k = (int)(ctx->issued % EV_RING);
  ctx->evProbe[k] = ctx->tagSlot;
  ctx->evGen[k] = ctx->probeGen;
  if (ctx->tagSlot >= 0) ctx->probeLast[ctx->tagSlot] = ctx->issued;
  ctx->tagSlot = -1;
  ctx->issued++;
  ctx->launches++;
}

// the RNG / Sobol sample index of frame frameCounter: sample-parallel ranks
// interleave their sample streams (rank r renders samples r, r+W, r+2W, ...)
static uint32_t sampleIndex(const pt_config& c, uint32_t frameCounter) {
  const uint32_t w = c.sample_world > 0 ? (uint32_t)c.sample_world : 1u;
  return frameCounter * w + (uint32_t)c.sample_rank;
}

SceneView sceneView(const pt_ctx* ctx) {
  SceneView s;
  s.geo = ctx->d_geo;
  s.pairs = ctx->d_pairs;
  s.hitRec = ctx->d_hit;
  s.mats = ctx->d_mats;
  s.nMats = ctx->nMats;
  s.bvh = ctx->d_bvh;
  s.nTop = std::min(LDS_NODES, ctx->nDevNodes);
  s.rootRef = ctx->rootRef;
  s.nTri = ctx->nTri;
  s.fast = 0;  // set per launch (renderFrame)
  s.fbvh = ctx->d_fbvh;
  s.fpairs = ctx->d_fpairs;
  s.fastTri = ctx->d_fastTri;
  s.fRoot = ctx->fRoot;
  s.fnTop = std::min(LDS_NODES, ctx->fnDev);
  s.fbvh4 = ctx->d_fbvh4;
  s.f4Root = ctx->f4Root;
  s.f4nTop = std::min(LDS_NODES * 4 / W4_F4, ctx->f4nDev);  // the LDS copy holds LDS_NODES * 4 float4
  s.refParent = ctx->d_refParent;
  s.refBox = ctx->d_refBox;
  s.leafBox = ctx->d_leafBox;
  return s;
}

// the uploaded environment as the kernels read it (rowTable: the sample table by rows, nt: Env::nt -- pt_plan.h)
Env envView(const pt_ctx* ctx, bool rowTable, int nt) {
  const EnvForms& v = ctx->env;
  Env e;
  e.hdr = v.hdr;
  e.cache = v.cache;
  e.hdr8 = v.hdr8;
  e.cache4 = v.cache4;
  e.cacheRow = rowTable ? v.cacheRow : nullptr;
  e.cacheY = rowTable ? v.cacheY : nullptr;
  e.trig = v.trig;
  e.light = v.light;  // every scene: c5 too (4.25 vs 4.49 ms without the table, round 6)
  e.w = v.w;
  e.h = v.h;
  e.res = v.w;
  e.nt = nt;
  return e;
}

// rank's share of a world-way screen-tile split of the context's image (the one place a Share is filled)
Share shareOf(const pt_ctx* ctx, int rank, int world) {
  return makeShare(ctx->cfg.width, ctx->cfg.height, ctx->shardSize, rank, world);
}

PackParams packParams(const pt_ctx* ctx, int rank, int world) {
  PackParams p;
  p.share = shareOf(ctx, rank, world);
  p.count = slots(p.share);
  return p;
}

// the caller's stream waits for the last update or clear of the tile planes when that ran on another
// stream (pt_set_stream since)
int joinAdaptive(pt_ctx* ctx) {
  if (ctx->adaptStream && ctx->adaptStream != ctx->stream) CK(hipStreamWaitEvent(ctx->stream, ctx->adaptDone, 0));
  return PT_OK;
}

// Every tile of a PT_FLAG_ADAPTIVE context active again, its error 0: on the caller's stream, after the
// running-mean updates of the launches so far (and so after their camera-ray passes), with adaptDone
// for the next pass of each slot. Nothing to clear (no update since the last clear) enqueues nothing.
static int clearAdaptive(pt_ctx* ctx) {
  ctx->adaptFrames = 0;
  if (!ctx->d_retiredAt || !ctx->adaptDirty) return PT_OK;
  if (int rc = joinPipe(ctx)) return rc;
  if (int rc = joinAdaptive(ctx)) return rc;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(hipMemsetAsync(ctx->d_retiredAt, 0, (size_t)ctx->adaptTiles * sizeof(uint32_t), ctx->stream));
  CK(hipMemsetAsync(ctx->d_err2, 0, (size_t)ctx->adaptTiles * sizeof(float), ctx->stream));
  CK(hipEventRecord(ctx->adaptDone, ctx->stream));
  ctx->adaptStream = ctx->stream;
  ctx->adaptGen++;
  ctx->adaptDirty = false;
  return PT_OK;
}

// the sample moments no longer describe the accumulation (it was replaced, or the scene or the
// light its samples saw): invalid until a launch restarts them at frameCounter 0
// ... and with them goes what adaptive sampling decided from them
int dropMoments(pt_ctx* ctx) {
  ctx->momFrames = 0;
  return clearAdaptive(ctx);
}

// make sure the overflow stack covers `threads` threads of a kernel keeping `ldsDepth` entries in LDS
static int ensureOverflow(pt_ctx* ctx, size_t threads, int* ovfDepth, int ldsDepth = LDS_STACK, int slots = 1) {
  // pt_trace.h StackT: at most maxStack - ldsDepth/2 - 1 entries are ever in HBM
  *ovfDepth = ctx->maxStack > ldsDepth ? ctx->maxStack - ldsDepth / 2 : 0;
  if (*ovfDepth == 0) return PT_OK;
  size_t need = threads * (size_t)(*ovfDepth) * (size_t)slots;  // slots: one region per frame in flight
  if (need > ctx->ovfInts) {
    dfree(ctx->d_ovf);
    CK(hipMalloc(&ctx->d_ovf, need * sizeof(int)));
    ctx->ovfInts = need;
  }
  return PT_OK;
}

// Two policies are chosen by measurement, since results are identical either
// way and which is faster depends on the scene and the integrator:
//  * the tree: the runtime's own (binned SAH; results checked against the
//    uploaded tree) pays off when the uploaded tree is poor -- the reference's
//    SAH with its z-typo: c2 0.57 -> 0.47 ms, c4 0.99 -> 0.80 -- and costs its
//    checks when the uploaded tree is already good (c5: +2 %);
//  * tile splitting (reorderKernel) pays off when the SIMDs have issue slots to
//    spare (the MIS integrator, latency-bound) and costs when they do not (the
//    Lambert megakernel is VALU-bound: a split item's idle lanes still take
//    issue cycles);
// (Longest-first tile order -- per-tile cost atomics, the order lookup of every
// claim, the reorder kernel -- was probed as well until round 5: it cost on the
// Lambert megakernel, c2 0.347 ms in band order vs 0.372, but Lambert frames run
// on the regen kernel now, and for the integrators left on the megakernel it
// never lost: c4 at N = 1 0.268 vs 0.267 ms, c4's 1/8 share in a 20-frame batch
// 0.072 vs 0.088, while the probe's noisy single-frame choice gave 0.069-0.087.)
// After a restart of the running mean (frameCounter 0, as on every camera move
// in the reference): frames 1-2 run the runtime's tree and 3-4 the uploaded
// one, unsplit; frame 5 runs the runtime's tree while the host, at frame 6,
// waits for frame 4 (frame 5 is already queued, so the GPU never drains) and
// keeps the faster tree; frames 6-10 split (the per-tile split state
// converges), 11-12 are timed, and at frame 14 -- waiting for frame 12 with 13
// queued -- the faster split policy is kept. No frame waits for its own
// predecessor. The decisions are kept across later restarts until the scene or
// the env is uploaded again (a camera move changes neither tree's merit nor,
// measurably, the split policy's), so only the first restart after an upload
// pays for the probe's slower trial frames; every restart still clears the
// per-tile split state and cost estimates. Sets *useFast; returns the split
// percentage for this frame's reorder (0 = off).
static int probePolicy(pt_ctx* ctx, uint32_t frameCounter, bool ordered, bool fastAllowed, bool* useFast, int slot,
                       hipStream_t S) {
  *useFast = fastAllowed;
  ctx->tagSlot = -1;
  if (!ordered) return 0;
  if (frameCounter == 0) {
    ctx->probeGen++;
    ctx->probeFrame = 0;
    for (int k = 0; k < 4; k++) {
      ctx->probeN[k] = 0;
      ctx->probeMs[k] = 0.0;
      ctx->probeLast[k] = -1;
    }
    const bool keep = ctx->treeDecided >= 0 && ctx->splitDecided >= 0 && ctx->probedKey == ctx->policyKey;
    if (!keep) ctx->treeDecided = ctx->splitDecided = -1;
    // Frames batched per launch (pipelined, RenderParams::nFrames) are not split. A batch's launch
    // holds each tile once per frame, so a costly tile's frames already run side by side, and split
    // items' idle lanes only cost issue slots: c4 without splitting 0.262 -> 0.251 ms at N = 1, its
    // 1/8 share 0.075 -> 0.070 ms (20 frames) and 0.054 -> 0.048 (200 frames, split at 50 %). A launch
    // of one frame (a display() call) is split when the probe found it faster.
    // (launchReorder applies the split only to launches of one frame, renderOne)
    ctx->probedKey = ctx->policyKey;
    // split state and cost estimates start over (the camera or scene changed), in every slot's
    // stream order (after its last reorder, before its next frame): this launch's slot on the stream
    // S it runs on (which may be the caller's, renderOne's solo launch), every other slot on its own
    // stream, with that slot's kernelDone recorded after the reset so that a later launch of the
    // slot issued solo on the caller's stream (only once every kernelDone has completed) follows it
    if (ctx->d_cost)
      for (int k = 0; k < (ctx->pipe ? ctx->pipeDepth : 1); k++) {
        const bool own = k == slot || !ctx->pipe;
        hipStream_t sk = own ? S : ctx->slotStream[k];
        (void)hipMemsetAsync(ctx->d_cost + (size_t)k * 4 * ctx->numItems + 2 * (size_t)ctx->numItems, 0,
                             2 * (size_t)ctx->numItems * sizeof(int), sk);
        if (!own && ctx->kernelDone[k]) {
          (void)hipEventRecord(ctx->kernelDone[k], sk);
          ctx->slotBusy[k] = true;
        }
      }
  }
  const int f = ctx->probeFrame < 1000 ? ctx->probeFrame++ : 1000;
  auto avg = [&](int k) { return ctx->probeN[k] ? ctx->probeMs[k] / ctx->probeN[k] : 1e30; };
  if (f == 6 && ctx->treeDecided < 0) {
    foldUpTo(ctx, std::max(ctx->probeLast[0], ctx->probeLast[1]));
    ctx->treeDecided = fastAllowed && avg(0) <= avg(1) ? 1 : 0;
  }
  if (f == 14 && ctx->splitDecided < 0) {
    foldUpTo(ctx, ctx->probeLast[2]);
    ctx->splitDecided = PT_SPLIT_PCT > 0 && avg(2) < avg(ctx->treeDecided ? 0 : 1) ? 1 : 0;
  }
  // this frame's tree, and the probe slot its time goes to
  if (ctx->treeDecided >= 0) {
    *useFast = fastAllowed && ctx->treeDecided;
  } else {
    *useFast = fastAllowed && (f <= 2 || f == 5);
    ctx->tagSlot = (f == 1 || f == 2) ? 0 : (f == 3 || f == 4) ? 1 : -1;
  }
  // this frame's split policy (for the next frame's items)
  if (ctx->splitDecided >= 0) return ctx->splitDecided ? PT_SPLIT_PCT : 0;
  if (f == 11 || f == 12) ctx->tagSlot = 2;
  return f >= 6 && f < 15 ? PT_SPLIT_PCT : 0;
}


// the slot streams (and their events) of depth D
static int ensureSlots(pt_ctx* ctx, int D) {
  for (int k = 0; k < D; k++) {
    if (!ctx->slotStream[k]) CK(hipStreamCreateWithFlags(&ctx->slotStream[k], hipStreamNonBlocking));
    if (!ctx->kernelDone[k]) CK(hipEventCreateWithFlags(&ctx->kernelDone[k], hipEventDisableTiming));
  }
  return PT_OK;
}

// the BASIC integrator's frame (BasicRayTracingWithC++): one kernel on the context's stream
static int renderBasic(pt_ctx* ctx, uint32_t frameCounter) {
  const pt_config& c = ctx->cfg;
  if (!ctx->d_shapes) return fail(ctx, PT_E_NOSCENE, "no BASIC shapes uploaded");
  const int maxDepth = maxBounce(c);  // B:254
  if (maxDepth > BASIC_MAX_DEPTH) return fail(ctx, PT_E_INVALID, "BASIC max_bounce > 31");
  if (int rc = ensureBasicImage(ctx)) return rc;
  if (!ctx->d_overruns) {
    CK(hipMalloc(&ctx->d_overruns, sizeof(unsigned long long)));
    CK(hipMemsetAsync(ctx->d_overruns, 0, sizeof(unsigned long long), ctx->stream));
  }
  hipEvent_t evb, eve;
  int erc = launchEvents(ctx, &evb, &eve);
  if (erc) return erc;
  BasicParams p;
  p.shapes = ctx->d_shapes;
  p.nShapes = ctx->nShapes;
  p.width = c.width;
  p.height = c.height;
  p.sample = sampleIndex(c, frameCounter);
  p.seed = c.basic_seed;
  p.maxDepth = maxDepth;
  p.reset = frameCounter == 0;
  p.brightness = (float)((double)(2.0f * 3.1415926f) * (1.0 / (double)c.basic_samples));  // B:20
  p.accum = ctx->d_accum;
  p.image = ctx->d_basicImg;
  p.stream = ctx->d_stream;
  p.offsets = ctx->d_offsets;
  p.streamN = ctx->streamN;
  p.nOffsets = ctx->nOffsets;
  p.stats = reinterpret_cast<unsigned long long*>(ctx->d_ctl + CTL_STATS);
  p.overruns = ctx->d_overruns;
  CK(hipEventRecord(evb, ctx->stream));
  CK(launchBasic(p, ctx->stream));
  CK(hipEventRecord(eve, ctx->stream));
  commitLaunch(ctx);
  return PT_OK;
}

// Where a launch runs. Pipelined, launch frameNo takes slot frameNo % depth (its stream, work-queue
// counters, overflow stack, tile order, camera-ray results and lists) and colour buffer
// frameNo % (2 * depth + 1); an unpiped context has one of each and runs on the context's stream.
struct FrameSlot {
  int D = 1, slot = 0, nCol = 3, colIdx = 0;
  // A launch issued while no other is in flight runs on the caller's stream itself: its camera-ray
  // pass, frame kernel and running-mean update -- and the caller's next work (the gather's pack) --
  // then follow one another in one queue instead of across queues (an event wait between hardware
  // queues costs ~15-18 us per hop; c2's 1/8 share of a 20-frame window is one launch)
  bool solo = false;
  hipStream_t S = nullptr;
};

// no slot's last launch is still running
static bool pipeIdle(pt_ctx* ctx, int D) {
  bool idle = true;
  for (int k = 0; k < D; k++)
    if (ctx->slotBusy[k] && hipEventQuery(ctx->kernelDone[k]) == hipErrorNotReady) idle = false;
  (void)hipGetLastError();  // hipEventQuery's not-ready status is not an error
  return idle;
}

// every other slot's frame in flight has ended on S (the frames that read buffers the launch rebuilds)
static int waitOthers(pt_ctx* ctx, const FrameSlot& at) {
  for (int k = 0; k < at.D; k++)
    if (k != at.slot && ctx->slotBusy[k]) CK(hipStreamWaitEvent(at.S, ctx->kernelDone[k], 0));
  return PT_OK;
}

// The launch shape: the kernel variant's block and blocks per CU (occupancy queries), and the grid.
struct LaunchShape {
  RegenShape rs;
  int bs = BLOCK;  // threads per block
  int fullGrid = 0, grid = 0;
};

static int gridFor(pt_ctx* ctx, const FramePlan& pl, const FrameSlot& at, LaunchShape* g) {
  const pt_config& c = ctx->cfg;
  int nb = 0;
  if (pl.regen) {
    CK(regenShape(c.integrator, pl.cull, pl.wide, pl.walk4 ? ctx->f4nDev : 0, !pl.wideScene, &g->rs));
    nb = g->rs.blocksPerCU;
  } else {
    CK(renderBlocksPerCU(c.integrator, pl.cull, pl.count, pl.wide, &nb));
  }
  if (nb < 1) nb = 1;
  g->bs = pl.regen ? g->rs.v.block : BLOCK;
  ctx->lastWaves = nb * g->bs / 64 / 4;  // 4 SIMDs per CU
  ctx->lastRegen = pl.regen;
  // Frames in flight share the GPU by space, not by time: a frame's persistent grid is
  // residency / (frames in flight), so the frames' waves are all resident together and a
  // frame whose long paths keep a few waves busy leaves the rest of the machine to the
  // others (and to the running-mean updates). A persistent grid sized to all of residency
  // keeps the next frame's waves -- and every other launch -- waiting for its tail: c4
  // 0.48 -> 0.34 ms per frame at 8 frames in flight, c2's 1/8 screen share 0.096 -> 0.072.
  // A caller that waits for every frame gets the whole machine for each.
  g->fullGrid = ctx->numCU * nb;
  g->grid = g->fullGrid;
  // While other frames are in flight, each frame's grid is PT_GRID_PCT % of its equal share: a frame
  // finishing early leaves waves of the others ready to take its place (round 4, against 100 /
  // 200 / 300 % with the bench line as the driver runs it, 20 frames from an idle GPU: c2 0.285 /
  // 0.262 / 0.266 / 0.289 ms per frame at 100 / 150 / 200 / 300, c4 0.413 / 0.360 / 0.367 / 0.385;
  // round 5's batched launches prefer 125, PT_GRID_PCT).
  // The share follows the launches actually in flight, PT_GRID_PCT % / (1 + the others running):
  // a launch issued into a filling pipeline (the first batches after an idle GPU) takes the
  // machine the earlier ones leave as they drain, and a full pipeline gets PT_GRID_PCT % / D each.
  // 20 frames from an idle GPU, one rank's share of an N-way split (profiles/r4/shard_time_h20.jsonl,
  // 2 runs each): c2 N = 4 0.129-0.130 -> 0.072 ms per frame, N = 8 0.061 -> 0.046-0.048, c4 N = 4
  // 0.137 -> 0.109-0.113; N = 1, 2 and 200-frame runs within run-to-run spread.
  const int GRID_PCT = pl.wideScene ? PT_GRID_PCT_WIDE : PT_GRID_PCT;
  if (pl.piped && at.D > 1) {
    int others = 0;  // other launches still in flight: the caller streams frames
    for (int k = 0; k < at.D; k++)
      others += k != at.slot && ctx->slotBusy[k] && hipEventQuery(ctx->kernelDone[k]) == hipErrorNotReady;
    (void)hipGetLastError();  // hipEventQuery's not-ready status is not an error
    if (others > 0)
      g->grid = std::min(g->fullGrid, std::max(NUM_QUEUES, g->fullGrid * GRID_PCT / (100 * (others + 1))));
  }
  return PT_OK;
}

// What the frame's kernels read of the context and the plan (the tree, the frames, the colour buffer,
// the tile order and the bins follow in renderOne)
static RenderParams fillParams(const pt_ctx* ctx, const FramePlan& pl, const FrameSlot& at, const LaunchShape& g,
                               int ovfDepth, const float eye[3], const float cameraRotate[16], uint32_t frameCounter) {
  const pt_config& c = ctx->cfg;
  RenderParams p;
  std::memset(&p, 0, sizeof(p));
  p.scene = sceneView(ctx);
  p.env = envView(ctx, pl.rowTable, pl.envNt);
  // the share's six fields, the rank's wave tiles (== ctx->numItems) and colStride: per-frame buffers are indexed
  // by the pixel's slot in this context's share (pt_frame.h slotOf), so a 1/N share's colour and camera-ray
  // buffers are 1/N of a frame (c5 at N = 8, 16 frames per launch: ~2.4 GB of colour buffers instead of ~19 GB)
  setShare(p, shareOf(ctx, c.tile_rank, c.tile_world));
  p.frameCounter = frameCounter;
  p.sampleIndex = sampleIndex(c, frameCounter);
  p.sampleStride = c.sample_world > 0 ? (uint32_t)c.sample_world : 1u;
  p.maxBounce = maxBounce(c);
  std::memcpy(p.eye, eye, sizeof(p.eye));
  std::memcpy(p.cam, cameraRotate, sizeof(p.cam));
  p.accum = ctx->d_accum;
  p.queue = reinterpret_cast<int*>(ctx->d_ctl + CTL_QUEUES) + (size_t)at.slot * NUM_QUEUES * CTL_LINE_INTS;
  p.perQueue = ctx->perQueue;
  p.ovf = ovfDepth ? ctx->d_ovf + (size_t)at.slot * g.fullGrid * g.bs * ovfDepth : nullptr;
  p.ovfDepth = ovfDepth;
  p.stats = reinterpret_cast<unsigned long long*>(ctx->d_ctl + CTL_STATS);
  p.rayShards = reinterpret_cast<unsigned long long*>(ctx->d_ctl + CTL_RAYS);
  return p;
}

// Longest-tiles-first: the slot's per-tile costs and its order list (both null: a launch in band order
// records no costs and launches no reorder)
static int tileOrderLists(pt_ctx* ctx, bool ordered, int slot, int** cost, int** order) {
  const int orderCap = 4 * ctx->perQueue + 64;  // room for the items of split tiles
  const size_t orderInts = (size_t)NUM_QUEUES * orderCap + NUM_QUEUES;
  ctx->orderCap = orderCap;
  if (!ordered) return PT_OK;
  if (!ctx->d_cost) {
    // per slot and tile: summed item cost, longest item, split state, cost estimate
    // (reorderKernel reads and zeroes the costs)
    const size_t n = (size_t)PIPE * ctx->numItems * 4;
    CK(hipMalloc(&ctx->d_cost, n * sizeof(int)));
    CK(hipMemset(ctx->d_cost, 0, n * sizeof(int)));
    // per slot and band: orderCap work items, then the NUM_QUEUES item counts (reorderKernel)
    CK(hipMalloc(&ctx->d_order, (size_t)PIPE * orderInts * sizeof(int)));
    for (int k = 0; k < PIPE; k++) ctx->orderValid[k] = false;
  }
  *cost = ctx->d_cost + (size_t)slot * 4 * ctx->numItems;
  *order = ctx->d_order + (size_t)slot * orderInts;
  return PT_OK;
}

// Camera-ray bins, rebuilt when the camera or the scene changed (the previous frame has ended
// first: it may still read the old bins), and with a camera-ray pass the slot's results and lists
// The one place that decides "a pipelined launch with bins and a pass" (p->col, set by the caller, and
// results to write): its pass runs over the bins' pass list and its running-mean update takes the
// other tiles' samples -- *sky is filled for both (binStart non-null), else left empty.
static int bindBins(pt_ctx* ctx, const FramePlan& pl, const FrameSlot& at, const RegenShape& rs, int nF,
                    const float eye[3], const float cameraRotate[16], RenderParams* p, SkyTiles* sky) {
  const pt_config& c = ctx->cfg;
  hipStream_t S = at.S;
  if (!ctx->binsValid || ctx->binVersion != ctx->sceneVersion || std::memcmp(ctx->binEye, eye, sizeof(ctx->binEye)) ||
      std::memcmp(ctx->binCam, cameraRotate, sizeof(ctx->binCam))) {
    if (pl.piped) {
      if (int e = waitOthers(ctx, at)) return e;
      // ... and the running-mean updates enqueued so far read the old bin starts (SkyTiles): the last one
      // follows the others on the caller's stream
      if (ctx->mixPending && S != ctx->lastMixStream) CK(hipStreamWaitEvent(S, ctx->mixDone[ctx->lastCol], 0));
    }
    ctx->binsValid = false;
    CK(buildPrimaryBins(eye, cameraRotate, c.width, c.height, ctx->d_geo, ctx->d_leafBox, ctx->nTri, ctx->bins, S));
    CK(buildPassList(shareOf(ctx, c.tile_rank, c.tile_world), ctx->bins, S));
    ctx->binBuilds++;
    std::memcpy(ctx->binEye, eye, sizeof(ctx->binEye));
    std::memcpy(ctx->binCam, cameraRotate, sizeof(ctx->binCam));
    ctx->binVersion = ctx->sceneVersion;
    ctx->binsValid = true;
    if (pl.piped) {
      CK(hipEventRecord(ctx->binsBuilt, S));
      ctx->binGen++;
      ctx->binGenSeen[at.slot] = ctx->binGen;
    }
  }
  // a frame in flight on the other slot's stream must not read bins still being built
  if (pl.piped && ctx->binGenSeen[at.slot] != ctx->binGen) {
    CK(hipStreamWaitEvent(S, ctx->binsBuilt, 0));
    ctx->binGenSeen[at.slot] = ctx->binGen;
  }
  p->binStart = ctx->bins.binStart;
  p->binTris = ctx->bins.binTris;
  p->binGeo = ctx->bins.binGeo;
  p->binBox = ctx->bins.binBox;
  p->binTilesX = ctx->bins.tilesX;
  p->binTilesY = ctx->bins.tilesY;
  if (!pl.pass) return PT_OK;
  const int n = pl.piped ? at.D : 0, cap = std::max(nF, pl.piped ? ctx->batchCap : 1);
  // the slot's previous launch (on S) may still read the old results and lists
  auto waitSlot = [&]() { return hipStreamSynchronize(S); };
  // per frame: the share's entries (colStride int2, compacted per wave tile), then its numItems tile masks
  const size_t primBytes = p->colStride * sizeof(int2) + (size_t)ctx->numItems * sizeof(unsigned long long);
  if (int rc = frameBuffer(ctx, ctx->d_prim, ctx->primCap, n, at.slot, nF, cap,
                           [&](int f) { return (size_t)f * primBytes; }, waitSlot))
    return rc;
  p->primHit = ctx->d_prim[at.slot];
  p->primMask = reinterpret_cast<unsigned long long*>(ctx->d_prim[at.slot] + (size_t)ctx->primCap[at.slot] * p->colStride);
  // (not on the scenes that outgrow the L2s: their persistent grids fill every CU for milliseconds, and the
  // longer update waits for room as every kernel beside them does -- c5 4.03 -> 4.13 ms per frame with the
  // rule; they keep the pass over every tile)
  if (p->col && p->primHit && !pl.wideScene) {
    sky->binStart = ctx->bins.binStart;
    sky->binTilesX = ctx->bins.tilesX;
    sky->sampleIndex = p->sampleIndex;
    sky->sampleStride = p->sampleStride;
    std::memcpy(sky->cam, cameraRotate, sizeof(sky->cam));
    sky->env = p->env;
    sky->rayShards = p->rayShards;
    // The pass leaves the masks of the tiles outside its list alone, and every reader of its results
    // (liveListKernel, primTileMask in the frame kernels) must find 0 there: the slot's whole mask region
    // is zeroed before the slot's first such launch with this bin build or this buffer. On S, so after the
    // slot's previous launch (its stream, or ordered before it: enqueueMix, pipeIdle) and before this pass;
    // each slot does it for itself, after its wait for binsBuilt. Until the next build the unlisted tiles are
    // the same ones, and a launch with the full grid writes them 0 as well (an empty bin leaves no path),
    // so the zeros hold.
    const int k = at.slot;
    if (ctx->maskBuild[k] != ctx->binBuilds || ctx->maskBuf[k] != ctx->d_prim[k] || ctx->maskCap[k] != ctx->primCap[k]) {
      CK(hipMemsetAsync(p->primMask, 0, (size_t)ctx->primCap[k] * ctx->numItems * sizeof(unsigned long long), S));
      ctx->maskBuild[k] = ctx->binBuilds;
      ctx->maskBuf[k] = ctx->d_prim[k];
      ctx->maskCap[k] = ctx->primCap[k];
    }
  }
  // the regen kernels claim from per-queue lists of the tiles the pass left paths in (all variants
  // but the large scenes' MIS one, pt_regen.hip regenLists)
  if (pl.regen && regenTakesLists(c.integrator, rs)) {
    // per slot, like the results: every queue's segment of live items (liveStride records of 16 bytes)
    if (int rc = frameBuffer(ctx, ctx->d_live, ctx->liveCap, n, at.slot, nF, cap,
                             [&](int f) { return (size_t)NUM_QUEUES * liveStride(ctx->perQueue, f) * sizeof(uint4); },
                             waitSlot))
      return rc;
    p->liveItems = p->primHit ? ctx->d_live[at.slot] : nullptr;  // (a share that owns no tile has no results and no lists)
  }
  return PT_OK;
}

// The launch's own kernels on its stream, between the launch's begin and end events: the slot's
// work-queue counters zeroed, the camera-ray pass and its lists, the frame kernel, the tile reorder
static int enqueueFrame(pt_ctx* ctx, const FramePlan& pl, const FrameSlot& at, const LaunchShape& g, RenderParams& p,
                        const SkyTiles& sky, int* cost, int* order, int split) {
  const pt_config& c = ctx->cfg;
  hipStream_t S = at.S;
  hipEvent_t evb, eve;
  int erc = launchEvents(ctx, &evb, &eve);
  if (erc) return erc;
#if PT_WAVE_TRACE
  // diagnostics build: each wave's {start, end, tiles | longest tile's pixel << 32,
  // longest tile's duration, its most node-loop / leaf-loop iterations of a lane} (100 MHz wall
  // clock), appended per frame to $PT_WAVE_TRACE_FILE (tools/wave_trace.py)
  const size_t nTrace = (size_t)g.grid * (g.bs / 64) * WAVE_TRACE_WORDS;
  unsigned long long* dTrace = nullptr;
  {
    CK(hipMalloc(&dTrace, nTrace * sizeof(unsigned long long)));
    CK(hipMemsetAsync(dTrace, 0, nTrace * sizeof(unsigned long long), S));
  }
  p.waveTrace = dTrace;
#endif
  // the pass over the bins' pass list (bindBins); an empty list launches no pass: every mask is 0 already
  const int* passList = sky.binStart ? ctx->bins.passList : nullptr;
  const bool passRuns = p.primHit && !(passList && ctx->bins.passCount == 0);
  // the slot's work-queue counters zeroed for this launch: by the camera-ray pass (block 0), else by a memset
  p.zeroQueue = passRuns;
  if (!passRuns) CK(hipMemsetAsync(p.queue, 0, (size_t)NUM_QUEUES * CTL_LINE_INTS * sizeof(int), S));
  CK(hipEventRecord(evb, S));
  if (passRuns) CK(launchPrimary(p, passList, ctx->bins.passCount, S));
  if (p.liveItems) CK(launchLiveList(p, S));  // the frame kernel claims only tiles the pass left paths in
  if (pl.regen) CK(launchRegen(p, c.integrator, g.grid, S, pl.cull, g.rs));
  else CK(launchRender(p, c.integrator, g.grid, S, pl.cull, pl.count, pl.wide));
#if PT_WAVE_TRACE
  if (dTrace) {
    std::vector<unsigned long long> tr(nTrace);
    CK(hipMemcpyAsync(tr.data(), dTrace, nTrace * sizeof(unsigned long long), hipMemcpyDeviceToHost, S));
    CK(hipStreamSynchronize(S));
    (void)hipFree(dTrace);
    if (const char* fn = std::getenv("PT_WAVE_TRACE_FILE")) {
      if (FILE* f = std::fopen(fn, "ab")) {
        std::fwrite(tr.data(), sizeof(unsigned long long), nTrace, f);
        std::fclose(f);
      }
    }
  }
#endif
  if (pl.ordered) {
    CK(launchReorder(cost, cost + ctx->numItems, cost + 2 * (size_t)ctx->numItems, cost + 3 * (size_t)ctx->numItems,
                     order, ctx->perQueue, ctx->orderCap, ctx->numItems, std::max(1, PT_TILE_GROUP),
                     g.grid * (BLOCK / 64), split, S));
    ctx->orderValid[at.slot] = true;
    ctx->orderSplit[at.slot] = split > 0;
  }
  // kernel_ms: the frame's own kernels (camera-ray pass, frame kernel, reorder), so the
  // policy probe weighs the order's cost too; the running-mean update is not in it
  CK(hipEventRecord(eve, S));
  return PT_OK;
}

// A pipelined launch's running-mean update: on the caller's stream, in frame order, after the
// launch's kernels (direct: the frame's kernels updated the running mean themselves)
static int enqueueMix(pt_ctx* ctx, const FrameSlot& at, int nF, bool direct, uint32_t frameCounter, const SkyTiles& sky) {
  const pt_config& c = ctx->cfg;
  const int slot = at.slot, colIdx = at.colIdx;
  const size_t shareN = (size_t)ctx->numItems * 64;
  CK(hipEventRecord(ctx->kernelDone[slot], at.S));
  ctx->slotBusy[slot] = true;
  if (at.S != ctx->slotStream[slot])  // the slot's resources: its stream's later work follows this launch
    CK(hipStreamWaitEvent(ctx->slotStream[slot], ctx->kernelDone[slot], 0));
  if (at.S != ctx->stream) CK(hipStreamWaitEvent(ctx->stream, ctx->kernelDone[slot], 0));
  if (ctx->mixPending && ctx->lastMixStream != ctx->stream)  // the caller switched streams: keep frame order
    CK(hipStreamWaitEvent(ctx->stream, ctx->mixDone[ctx->lastCol], 0));
  ctx->lastMixStream = ctx->stream;
  if (ctx->d_mom) {
    if (ctx->d_retiredAt) {
      // the retired tiles' pixels left alone: the state this launch's camera-ray pass saw (an update or
      // a clear since then would be enqueued after this, on this stream -- or on the one the caller left)
      if (int rc = joinAdaptive(ctx)) return rc;
      CK(launchMixAdaptive(packParams(ctx, c.tile_rank, c.tile_world), ctx->d_accum, ctx->d_mom, ctx->d_col[colIdx],
                           shareN, nF, frameCounter, ctx->d_retiredAt, sky, ctx->stream));
    } else {
      CK(launchMixMoments(packParams(ctx, c.tile_rank, c.tile_world), ctx->d_accum, ctx->d_mom, ctx->d_col[colIdx],
                          shareN, nF, frameCounter, sky, ctx->stream));
    }
    // the frames the moments hold: a restart, a continuation, or a gap (not valid)
    ctx->momFrames = frameCounter == 0 ? (uint32_t)nF : (frameCounter == ctx->momFrames ? ctx->momFrames + (uint32_t)nF : 0u);
  } else if (!direct)
    CK(launchMix(packParams(ctx, c.tile_rank, c.tile_world), ctx->d_accum, ctx->d_col[colIdx], shareN, nF,
                 frameCounter, sky, ctx->stream));
  CK(hipEventRecord(ctx->mixDone[colIdx], ctx->stream));  // direct: the frame's kernels updated it
  ctx->lastSlot = slot;
  ctx->lastCol = colIdx;
  ctx->mixPending = true;
  ctx->frameNo++;
  return PT_OK;
}

// One launch: frame frameCounter, or -- pipelined, with no policy probe running and the batch
// not starting a running mean -- up to `want` consecutive frames of the same camera
// (RenderParams::nFrames, at most ctx->batchCap). *done = the frames rendered.
static int renderOne(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t frameCounter,
                     int want = 1, int* done = nullptr) {
  if (!ctx) return PT_E_INVALID;
  if (done) *done = 1;
  CK(hipSetDevice(ctx->cfg.device_id));
  const pt_config& c = ctx->cfg;
  if (c.integrator == PT_BASIC_CPU_COMPAT) return renderBasic(ctx, frameCounter);
  if (!ctx->d_bvh || !eye || !cameraRotate) return fail(ctx, ctx->d_bvh ? PT_E_INVALID : PT_E_NOSCENE, "no scene");
  // where the launch runs, and what it uses
  FrameSlot at;
  const bool piped = pipedFrames(ctx);
  if (piped) {
    if (int e = ensureSlots(ctx, ctx->pipeDepth)) return e;
    at.D = ctx->pipeDepth;
    at.slot = (int)(ctx->frameNo % (unsigned)at.D);
    at.nCol = 2 * at.D + 1;
    at.colIdx = (int)(ctx->frameNo % (unsigned)at.nCol);
    at.solo = ctx->solo && pipeIdle(ctx, at.D);
  }
  const bool eyeIn = eyeInDomain(ctx, eye);  // else this launch runs without the runtime tree (pt_plan.h)
  const FramePlan pl = planFrame(ctx, at.solo, want, eyeIn);
  const hipStream_t S = at.S = piped && !at.solo ? ctx->slotStream[at.slot] : ctx->stream;
  LaunchShape g;
  if (int rc = gridFor(ctx, pl, at, &g)) return rc;
  int ovfDepth = 0;
  if (int rc = ensureOverflow(ctx, (size_t)g.fullGrid * g.bs, &ovfDepth, pl.regen ? regenLdsStack() : LDS_STACK, at.D))
    return rc;
  // the colour buffer's previous launch (nCol back) has been mixed (the slot's queue counters,
  // order list and camera-ray results belong to its previous launch on this same stream)
  if (piped && ctx->frameNo >= (unsigned long long)at.nCol && !(S == ctx->stream && ctx->lastMixStream == S))
    CK(hipStreamWaitEvent(S, ctx->mixDone[at.colIdx], 0));
  RenderParams p = fillParams(ctx, pl, at, g, ovfDepth, eye, cameraRotate, frameCounter);
  int *cost = nullptr, *order = nullptr;
  if (int rc = tileOrderLists(ctx, pl.ordered, at.slot, &cost, &order)) return rc;
  // the tree (the runtime's own, checked against the uploaded one, unless asked
  // not to) and the split policy: probePolicy
  bool useFast = false;
  // (a probe that times such a launch compares the uploaded tree with itself: its decisions are not kept
  // past the next restart)
  if (!eyeIn) ctx->policyKey++;
  const int splitPct = probePolicy(ctx, frameCounter, pl.ordered,
                                   !pl.count && !pl.regen && ctx->fastReady && eyeIn && !(c.flags & PT_FLAG_REFERENCE_TREE),
                                   &useFast, at.slot, S);
  // the large-scene regen kernel walks the 4-wide runtime tree (checked against the uploaded one)
  if (pl.regen && pl.walk4) useFast = true;
  if (pl.regen && pl.wide)  // its own LDS copy's size: the top of the tree, or all of it
    p.scene.f4nTop = g.rs.fullTree ? ctx->f4nDev : std::min(regenTop4(g.rs, c.integrator), ctx->f4nDev);
  p.scene.fast = useFast ? 1 : 0;
  ctx->lastFast = useFast;
  p.packets = (useFast ? ctx->fDepth : ctx->depth) + 1 <= PKT_DEPTH;
  // While the policy probe times frames (probePolicy, 20 frames after a restart) a pipelined
  // frame starts only after the previous one has ended, and each launch is one frame.
  const bool probing = pl.ordered && (ctx->treeDecided < 0 || ctx->splitDecided < 0);
  const int nF = piped && !probing ? std::max(1, std::min(want, ctx->batchCap)) : 1;
  if (done) *done = nF;
  p.nFrames = nF;
  // One megakernel frame issued while no other launch is in flight (a display() call, SURVEY 8(d)'s
  // per-call time): the kernel mixes each pixel's sample into the running mean itself (IS:868-871;
  // one writer per pixel, the previous frame's update is ordered before it on the caller's stream)
  // -- no colour buffer round trip and no running-mean update launch: c4 per call 0.785 -> 0.772 ms.
  // The regen kernel keeps the update launch: the read of the running mean at each path's end stalls
  // its lock-step waves (c2 0.455 either way, c3 0.578 -> 0.587 ms)
  // A PT_FLAG_MOMENTS context never does: its samples pass through the colour buffer to mixMomentsKernel.
  const bool direct = piped && at.solo && nF == 1 && !pl.regen && !ctx->d_mom;
  if (direct && ctx->mixPending && ctx->lastMixStream != S) CK(hipStreamWaitEvent(S, ctx->mixDone[ctx->lastCol], 0));
  if (piped) {
    // its last frames' running-mean update has read the colour buffer
    if (int rc = frameBuffer(ctx, ctx->d_col, ctx->colCap, at.nCol, at.colIdx, nF, std::max(nF, ctx->batchCap),
                             [&](int f) { return (size_t)f * p.colStride * COL_F * sizeof(float); },
                             [&]() { return hipEventSynchronize(ctx->mixDone[at.colIdx]); }))
      return rc;
  }
  p.col = piped && !direct ? ctx->d_col[at.colIdx] : nullptr;
  if (ctx->d_retiredAt) {
    // a restart has every tile active again; the launch's pass runs after the last update or clear
    if (frameCounter == 0)
      if (int rc = clearAdaptive(ctx)) return rc;
    if (ctx->adaptGenSeen[at.slot] != ctx->adaptGen) {
      CK(hipStreamWaitEvent(S, ctx->adaptDone, 0));
      ctx->adaptGenSeen[at.slot] = ctx->adaptGen;
    }
    p.retiredAt = ctx->d_retiredAt;
  }
  SkyTiles sky;  // the tiles the running-mean update shades (bindBins); empty: none
  std::memset(&sky, 0, sizeof(sky));
  if (pl.bins)
    if (int rc = bindBins(ctx, pl, at, g.rs, nF, eye, cameraRotate, &p, &sky)) return rc;
  // a frame in band order (probePolicy) records no costs and launches no reorder; the
  // slot's last order list stays valid for its next ordered frame (any list covers every tile)
  // Batches of frames run unsplit (probePolicy) -- also on small screen-tile shares, whose launch lasts
  // about as long as its longest unsplit tile (c4's 1/8 share, 20 frames in one 1.3 ms launch: single
  // 8x8 tiles of 1.2-1.5 ms): splitting there measured c4 N = 8 0.0726 -> 0.0688 ms per frame over 20
  // frames but 0.0484 -> 0.0549 over 200, N = 4 0.0867 -> 0.0962 (round 6, not kept)
  const bool splitThis = nF == 1;
  // (a batch does not run the split items a one-frame launch's reorder listed: band order, once)
  p.tileOrder = pl.ordered && ctx->orderValid[at.slot] && !(!splitThis && ctx->orderSplit[at.slot]) ? order : nullptr;
  p.orderCap = ctx->orderCap;
  p.tileCost = cost;
  p.tileCostMax = pl.ordered ? cost + ctx->numItems : nullptr;
  if (piped && probing) {
    if (int e = waitOthers(ctx, at)) return e;
  }
  if (int rc = enqueueFrame(ctx, pl, at, g, p, sky, cost, order, splitThis ? splitPct : 0)) return rc;
  if (piped)
    if (int rc = enqueueMix(ctx, at, nF, direct, frameCounter, sky)) return rc;
  commitLaunch(ctx, nF);
  return PT_OK;
}

// the caller's stream waits for the last pipelined frame's running-mean update
int joinPipe(pt_ctx* ctx) {
  if (!ctx->mixPending) return PT_OK;
  CK(hipSetDevice(ctx->cfg.device_id));
  CK(hipStreamWaitEvent(ctx->stream, ctx->mixDone[ctx->lastCol], 0));
  return PT_OK;
}

// every stream the context renders on, then its own: all work done
int syncStreams(pt_ctx* ctx) {
  CK(hipSetDevice(ctx->cfg.device_id));
  for (int k = 0; k < PIPE; k++) {
    if (ctx->slotStream[k]) CK(hipStreamSynchronize(ctx->slotStream[k]));
    ctx->slotBusy[k] = false;
  }
  CK(hipStreamSynchronize(ctx->stream));
  ctx->mixPending = false;
  return PT_OK;
}

int pt_render_frames_async(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t frameCounter,
                           int nFrames) {
  if (!ctx || nFrames < 0) return PT_E_INVALID;
  while (nFrames > 0) {
    int done = 1;
    if (ctx->peers.empty()) {
      if (int rc = renderOne(ctx, eye, cameraRotate, frameCounter, nFrames, &done)) return rc;
    } else {
      // a device group: every device renders its tiles of the frame on its own stream; then the
      // gather (GroupGather), frame by frame
      for (pt_ctx* m : members(ctx))
        if (int rc = renderOne(m, eye, cameraRotate, frameCounter)) return fromPeer(ctx, m, rc);
      if (int rc = groupGather(ctx)) return rc;
    }
    frameCounter += (uint32_t)done;
    nFrames -= done;
  }
  return PT_OK;
}

int pt_render_frame_async(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t frameCounter) {
  return pt_render_frames_async(ctx, eye, cameraRotate, frameCounter, 1);
}

int pt_render_frame(pt_ctx* ctx, const float eye[3], const float cameraRotate[16], uint32_t frameCounter,
                    float* accum_rgba) {
  int rc = pt_render_frame_async(ctx, eye, cameraRotate, frameCounter);
  if (rc) return rc;
  if (accum_rgba) return pt_download_accum(ctx, accum_rgba);
  return pt_synchronize(ctx);
}
