// pt_runtime.h -- what the host files of the C-ABI share: the context, the error helpers, and the
// functions one file defines and another calls. The files, by subject: pt_context.cpp (context life,
// streams, stats), pt_scene_upload.cpp (scene upload, geometry and material updates), pt_env.cpp
// (environment upload and update, BASIC state), pt_runtime.cpp (the frame path), pt_queries.cpp (ray
// and radiance queries), pt_accum.cpp (accumulation access, adaptive sampling, pack and unpack),
// pt_group.cpp (the in-process device group) and pt_post.cpp (the display post-processing).
// Internal: not installed.
// (The launch policy of the frame path -- pure functions of this context -- is pt_plan.h; the
// host-only scene preparation, which does not know the context, is pt_scene_prep.h; what the in-place
// updates of pt_scene_upload.cpp and pt_env.cpp share is pt_update.h; the environment's buffers and the
// view of them the kernels get are pt_envupdate.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pt_abi.h"
#include "pt_envupdate.h"
#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_rccl.h"

using namespace pt;

static constexpr int EV_RING = 64;
// Frames in flight: the default megakernel's (or regen kernel's) launch g (its pipeline
// sequence number) runs on slot stream g % depth (8 by default) with its own work queues,
// overflow stack, tile order and camera-ray results, and writes its sample colours to colour
// buffer g % (2 * depth + 1). While k other launches are in flight its persistent grid is 1.5 /
// (k + 1) of residency (gridFor), so the frames in flight share the GPU by space: their waves
// are resident together, and a frame whose last long paths keep a few waves busy leaves the
// rest of the machine to the others. Its running-mean update (mixKernel) runs on the caller's
// stream, in frame order, once the launch's kernel has ended: the accumulation is updated in
// frame order, the image is bit for bit the one of serial frames, and whatever the caller
// queues behind a frame (pack, download, tonemap) follows its update with no further
// cross-queue wait. No launch waits for a mix except the one of the launch 2 * depth + 1 back,
// whose colour buffer it reuses.
//
// A launch may render a batch of consecutive frames of one camera (pt_render_frames_async,
// RenderParams::nFrames): every frame's colours in its own part of the colour buffer, and one
// mixKernel folds them into the running mean pixel by pixel in frame order. A small screen-tile
// share (1/8 of the image) gives one frame too little work to fill the machine; a batch of
// tile_world frames per launch is about one whole image's work, and the chain of running-mean
// updates on the caller's stream -- one cross-queue wait and one launch per update, which set
// an 8-way share's frame period before -- has one link per batch.
// (Measured alternatives, DESIGN.md 4: a separate mix stream is twice as slow at small
// shares -- each mix waited on two ~25 us cross-queue signals in a chain from mix to mix; and
// with full-residency grids a mix waits for a CU slot behind the next frame's persistent
// kernel, ~250 us on c2, which made deeper pipelines slower, not faster.)
#ifndef PT_PIPE
#define PT_PIPE 8  // frames in flight (PT_PIPE_DEPTH overrides; capped by the hardware queues)
#endif
static constexpr int PIPE = MAX_SLOTS;      // most frames in flight
// colour buffers: a launch reuses the buffer of the launch 2 * depth + 1 back, whose running-mean
// update is then long done -- with depth + 1 the wait made a slot's next frame follow the
// running-mean update of the previous frame on another slot (two cross-queue hops), and an N = 8
// share of c2 kept only ~3 of its 8 frames in flight
static constexpr int COLS = 2 * MAX_SLOTS + 1;

struct pt_ctx {
  pt_config cfg{};
  std::string err;
  hipStream_t own = nullptr, stream = nullptr;
  // Launch timing: a fixed ring of begin/end event pairs. Launch number i (since
  // pt_create) records into pair i % EV_RING; a launch's elapsed time is folded
  // into the running totals once its end event has completed (non-blocking on
  // every new launch, blocking only when the ring is full or stats are read), so
  // the cost per frame stays constant however long a caller renders.
  hipEvent_t ev[2 * EV_RING] = {};
  int evProbe[EV_RING] = {};    // probe slot of the launch in each ring position (-1 none)
  int evGen[EV_RING] = {};      // probe generation it was tagged in
  long long issued = 0, folded = 0;
  double msTotal = 0.0;         // summed device time of the folded launches since the reset
  float msLast = 0.0f;          // device time of the last folded launch
  int launches = 0;             // render launches since the reset
  long long frames = 0;         // frames those launches rendered (a batch launch renders several)
  int tagSlot = -1;             // probe slot for the launch being issued (probePolicy)
  int numCU = 0;
  // scene
  float4* d_geo = nullptr;
  float4* d_pairs = nullptr;  // triangles i and i+1 component-interleaved (SceneView::pairs)
  float4* d_hit = nullptr;   // per triangle: normals + material id (SceneView::hitRec)
  float4* d_mats = nullptr;  // the distinct materials (SceneView::mats)
  int nMats = 0;
  float4* d_bvh = nullptr;
  int nDevNodes = 0;  // internal nodes in d_bvh (device ids 0..nDevNodes-1)
  // the runtime's own tree (uploadAccel; SceneView::fast) and the reference
  // facts its results are checked against
  bool fastReady = false;
  float4* d_fbvh = nullptr;
  float4* d_fpairs = nullptr;
  int* d_fastTri = nullptr;
  int* d_refParent = nullptr;
  float4* d_refBox = nullptr;
  float4* d_leafBox = nullptr;
  int fRoot = REF_NONE, fnDev = 0, fDepth = 0;
  // the same tree collapsed to 4-wide nodes (encodeWide4; the large-scene regen kernel)
  float4* d_fbvh4 = nullptr;
  bool fast4Ready = false;
  int f4Root = REF_NONE, f4nDev = 0, f4Depth = 0;
  // the origin domain of the runtime tree in place (pt_kernels.h originInDomain): PT_ORIGIN_K x the scale
  // its boxes were widened by, set with every build of it (an upload's, a geometry update's rebuild)
  float originLimit = 0.0f;
  // the last pt_upload_scene (pt_frame_stats upload_ms, accel_*)
  float uploadMs = 0.0f, accelMs = 0.0f;
  int accelDevice = -1, accelNodes = 0, accelDepth = 0;
  int rootRef = REF_NONE;
  // pt_update_geometry: the uploaded tree's topology, kept on the host from the upload (8 bytes per
  // node, 4 per device wide node); the device tables (pt_kernels.h RefitTables) and the staging of the
  // host form's vertex records are made at the first update, so a context that never updates pays no
  // device memory for them (d_refBox, the boxes the refit starts from, is uploaded with every scene)
  std::vector<int2> refTopo;    // RefitTables::topo
  std::vector<int> refOrder;    // device wide node id -> reference node id (encodeWideTree's order)
  std::vector<int> refitStart;  // RefitTables::heightStart on the host
  RefitTables refit;
  float* d_updVerts = nullptr;  // nTri x 18 f32
  bool sceneFast = false;       // the upload prepared a runtime tree (SceneHost::fast)
  // pt_update_materials: the update's device tables (pt_kernels.h MaterialTables) and, in place of the
  // upload's d_mats, a table with room for one material per triangle, both made at the scene's first
  // material update; the host form's staging of the records at its first use
  MaterialTables matTab;
  float* d_updMats = nullptr;   // nTri x 18 f32
  int nTri = 0, nNodes = 0, depth = 0, maxStack = 0;
  size_t sceneBytes = 0;  // the scene's records on the device (pt_plan.h sceneBytes, largeScene)
  // env (pt_envupdate.h): the store owns every env buffer, pt_upload_env's and pt_update_env's alike; env is
  // the view of it the kernels get (envView), made by envForms and installed by setEnvForms alone, its size
  // also in hdrW / hdrH for the launch policy (pt_plan.h rowTable). releaseEnv empties all of it.
  EnvStore envStore;
  EnvForms env;
  int hdrW = 0, hdrH = 0;  // env.w, env.h
  // BASIC shapes, the double image, the replayed random stream
  double* d_shapes = nullptr;
  int nShapes = 0;
  double* d_basicImg = nullptr;
  double* d_stream = nullptr;
  long long* d_offsets = nullptr;
  long long streamN = 0, nOffsets = 0;
  unsigned long long* d_overruns = nullptr;
  // frame state
  float4* d_accum = nullptr;
  // control block (pt_kernels.h CTL_*): padded queue counters (zeroed per
  // launch), cumulative fetch stats, padded sharded cumulative ray counters
  unsigned char* d_ctl = nullptr;
  int* d_ovf = nullptr;
  int* d_cost = nullptr;   // per slot: per-tile cost of its last frame, longest item, split state, estimate
  int* d_order = nullptr;  // per slot: per-band work items for its next frame
  bool lastFast = false;    // the last megakernel frame traversed the runtime's tree
  bool lastRegen = false;   // the last frame ran the path-regeneration kernel
  int lastWaves = 0;        // waves per SIMD of the last megakernel launch (occupancy query)
  // tree / tile-split policy probe (probePolicy): frames since the probe (re)started,
  // the summed frame times of each policy, the decision
  int probeFrame = 0;
  // camera-ray bins (pt_primary.hip) of the camera and scene they were built for
  PrimaryBins bins;
  bool binsValid = false;
  float binEye[3] = {}, binCam[16] = {};
  unsigned sceneVersion = 0, binVersion = 0;
  // frames in flight (PIPE slots; see PIPE above)
  bool pipe = false;                        // this context pipelines its megakernel frames
  int pipeDepth = PT_PIPE;                  // frames in flight (slot streams in use), 1..PIPE
  int pipeDepthBase = PT_PIPE;              // ... as chosen at creation (uploadScene may lower it for large scenes)
  bool pipeDepthFixed = false;              // PT_PIPE_DEPTH set: no scene-dependent choice
  // Frames of one pt_render_frames_async call rendered per launch (RenderParams::nFrames), at most:
  // pt_config.frame_batch, else as many as make one launch about a whole image's work (tile_world
  // frames of a screen-tile share, up to MAX_BATCH). Probe frames and frameCounter 0 run alone.
  int batchCap = 1;
  int colCap[COLS] = {};                    // frames each colour buffer holds
  int primCap[PIPE] = {};                   // frames each slot's camera-ray results hold
  int liveCap[PIPE] = {};                   // ... and each slot's live-item lists (regen kernels)
  // the large-scene path (regen kernel at 4 waves/SIMD, 4-wide walk with dynamic ray fetch,
  // camera-ray pass) on scenes of any size: -1 = for the Lambert integrator (c2 0.342 ->
  // 0.251 ms/frame) and the MIS integrator at 2 bounces (round 5: c3 0.1443 -> 0.1331; c4's 8
  // bounces keep the megakernel); PT_FLAG_REGEN / PT_FLAG_MEGAKERNEL choose per context,
  // PT_REGEN_WIDE = 1 / 0 (environment) for every / no scene
  int regenWide = -1;
  bool solo = true;                         // PT_SOLO = 0 (environment): every pipelined launch on a slot stream
  hipStream_t slotStream[PIPE] = {};
  hipEvent_t kernelDone[PIPE] = {};         // slot's last frame kernel (+ reorder) ended
  bool slotBusy[PIPE] = {};                 // kernelDone[k] has been recorded since the last sync
  hipEvent_t mixDone[COLS] = {};            // colour buffer's last running-mean update
  hipStream_t lastMixStream = nullptr;      // the stream the last update ran on (pt_set_stream may change it)
  // camera-ray bins built on one slot's stream: binsBuilt is recorded after the build, and
  // every other slot waits for it once before its first frame with those bins (binGen)
  hipEvent_t binsBuilt = nullptr;
  unsigned binGen = 0, binGenSeen[MAX_SLOTS] = {};
  // A pipelined launch's camera-ray pass visits only the tiles of bins.passList, so the other tiles' masks
  // in the slot's results must be zeros already: the slot's mask region is zeroed when the slot first takes
  // such a launch with a new bin build (binBuilds) or a (re)allocated d_prim (bindBins)
  unsigned binBuilds = 0, maskBuild[PIPE] = {};
  const void* maskBuf[PIPE] = {};
  int maskCap[PIPE] = {};
  float* d_col[COLS] = {};                  // per-colour-buffer sample colours (COL_F floats per slot)
  int2* d_prim[PIPE] = {};                  // per-slot camera-ray results (primaryKernel)
  uint4* d_live[PIPE] = {};                 // per-slot live-item lists and their counts (liveListKernel)
  int lastSlot = -1;                        // slot of the last pipelined frame
  int lastCol = -1;                         // colour buffer of the last pipelined frame
  bool mixPending = false;                  // a pipelined frame's update may still be running
  unsigned long long frameNo = 0;           // pipelined frames issued
  int probeN[4] = {0, 0, 0, 0};        // timed frames: runtime tree, uploaded tree (both unsplit), split
  double probeMs[4] = {0.0, 0.0, 0.0, 0.0};
  long long probeLast[4] = {-1, -1, -1, -1};  // launch number of each slot's last timed frame
  int probeGen = 0;
  int treeDecided = -1, splitDecided = -1;  // -1 probing, 0 off, 1 on
  unsigned policyKey = 0, probedKey = ~0u;  // bumped by every scene / env upload; the key the decisions were made for
  int orderCap = 0;        // work items per band in d_order
  bool orderValid[PIPE] = {};
  bool orderSplit[PIPE] = {};               // the slot's order list holds split items (a one-frame launch built it)
  size_t ovfInts = 0;
  // shards
  int shardSize = 32, shardsX = 0, shardsY = 0, numItems = 0, perQueue = 0;
  // scratch for tonemap
  float* d_rgb = nullptr;
  // The ray queries on device memory (pt_trace_closest_device, pt_trace_occluded_device, pt_radiance_device and
  // their host forms): their own stack overflow area, sized at first use for the largest grid a query launches and
  // for the tree depth of the scene (again after an upload that deepens it), so a query
  // never aliases a frame in flight (d_ovf) and allocates nothing in the steady state. queryDone is
  // recorded behind every query: a query on another stream (pt_set_stream since) waits for it -- the
  // area is one query's at a time -- and so does a resize.
  int* d_queryOvf = nullptr;
  size_t queryOvfInts = 0;
  hipEvent_t queryDone = nullptr;
  hipStream_t queryStream = nullptr;  // the stream queryDone was last recorded on
  bool queryIssued = false;
  float* d_queryStage = nullptr;      // the host forms' staging: rays, bounds (or ids) and results of one call
  size_t queryStageFloats = 0;
  // guide buffers of the last pt_render_guides (valid for the scene version they were traced in) and
  // the denoiser's images: two ping-pong colour planes, their tone-mapped planes, and the
  // image the last pt_denoise wrote (one of the two, or the caller's)
  float4* d_guide[3] = {};   // pos_t, nrm_tri, albedo of the current set (guideSet)
  // pos_t / nrm_tri exist twice: pt_temporal_commit marks the current set as the history's, and
  // pt_render_guides then writes the other one (albedo is not part of the history: one plane)
  float4* d_guidePN[2][2] = {};
  int guideSet = 0;
  float guideEye[3] = {}, guideCam[16] = {};  // the camera of the current guides
  bool guidesValid = false;
  unsigned guideVersion = 0;
  int* d_guideOvf = nullptr;  // the guide kernel's own stack overflow area (frames in flight use d_ovf)
  size_t guideOvfInts = 0;
  float4* d_dn[2] = {};
  float4* d_dnTm[2] = {};
  const float4* denoised = nullptr;
  // the temporal resolve: two resolved planes (the one the last resolve wrote and, after a commit,
  // the history's), the image the last resolve wrote (one of the two, or the caller's), the history
  float4* d_res[2] = {};
  int resCur = 0;                  // the plane the next context-owned resolve writes
  const float4* resolved = nullptr;
  bool resolvedFresh = false;      // a resolve since the last commit / reset / pt_render_guides
  bool histValid = false;
  int histSet = 0, histRes = 0;    // the history's guide set and resolved plane
  float histEye[3] = {}, histCam[16] = {};
  // PT_FLAG_MOMENTS: the running means (m1, m2) of the sample luminance beside the running mean of
  // the colour (mixMomentsKernel), and the frames they hold (0: not valid, see noteMoments)
  float2* d_mom = nullptr;
  uint32_t momFrames = 0;
  // PT_FLAG_ADAPTIVE (pt_adaptive.hip): per 8x8 tile of the image (ty * adaptTilesX + tx) the error the last
  // pt_adaptive_update found and the frame count at which the tile retired (0: active), allocated and
  // zeroed at creation. The update writes them on the caller's stream after every earlier launch's
  // running-mean update (so every earlier camera-ray pass has read them); adaptDone is recorded after
  // it, and every slot waits for it once before its next pass (adaptGen, like the bins)
  float* d_err2 = nullptr;
  uint32_t* d_retiredAt = nullptr;
  int adaptTilesX = 0, adaptTiles = 0;
  uint32_t adaptFrames = 0;         // momFrames at the last update (0: none since the restart)
  bool adaptDirty = false;          // an update since the planes were last zero: a restart has something to clear
  hipEvent_t adaptDone = nullptr;
  hipStream_t adaptStream = nullptr;  // the stream adaptDone was last recorded on
  unsigned adaptGen = 0, adaptGenSeen[MAX_SLOTS] = {};
  // pt_denoise_var: l = lum(tm(input)), step A's variance, the passes' two (l, v) planes
  float* d_lum = nullptr;
  float* d_var0 = nullptr;
  float2* d_lv[2] = {};
  bool varianceValid = false;  // d_var0 holds the last pt_denoise_var's step A
  // in-process multi-GPU (pt_config.n_devices > 1): this context renders as
  // screen-tile rank 0 on device_ids[0] and owns the other ranks' contexts and
  // the per-frame gather of their tiles into its accumulation
  std::vector<pt_ctx*> peers;  // ranks 1 .. n_devices-1
  struct GroupGather* gather = nullptr;
};

// The per-frame gather of an in-process device group. Rank k >= 1 packs its
// tiles (packKernel) on its render stream into one of two send buffers; the
// packed tiles travel to rank 0's device -- an RCCL send/recv group over the
// communicator of all the devices, or hipMemcpyPeerAsync -- and are unpacked
// into rank 0's accumulation on rank 0's communication stream. Rank 0's next
// frame renders meanwhile (its own tiles only); a send buffer is packed again
// only after its previous transfer completed.
struct GroupGather {
  int mode = PT_GATHER_COPY;
  int n = 0;
  hipStream_t cstream = nullptr;  // rank 0's device: receives, copies, unpacks
  hipEvent_t done = nullptr;      // rank 0's device: the last frame's unpacks
  bool pending = false;
  unsigned frame = 0;
  struct Peer {
    int dev = 0;
    size_t count = 0;                       // packed pixels (float4) of this rank
    float* send[2] = {nullptr, nullptr};    // on the rank's device, PACK_F floats per slot
    float* recv = nullptr;                  // on rank 0's device
    hipStream_t mstream = nullptr;          // the rank's device: RCCL sends
    hipEvent_t packed[2] = {nullptr, nullptr};
    hipEvent_t sent[2] = {nullptr, nullptr};  // the buffer's transfer completed
    bool sentValid[2] = {false, false};
  };
  std::vector<Peer> peer;  // ranks 1 .. n-1
  ncclComm_t comms[PT_MAX_DEVICES] = {};
  bool commsReady = false;
};

#define CK(expr)                                                                     \
  do {                                                                               \
    hipError_t e_ = (expr);                                                          \
    if (e_ != hipSuccess) {                                                          \
      ctx->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
      return PT_E_HIP;                                                               \
    }                                                                                \
  } while (0)

static inline int fail(pt_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

template <class T>
static void dfree(T*& p) {
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

// every context of a device group (rank 0 first), or just ctx
static inline std::vector<pt_ctx*> members(pt_ctx* ctx) {
  std::vector<pt_ctx*> m{ctx};
  m.insert(m.end(), ctx->peers.begin(), ctx->peers.end());
  return m;
}

static inline int fromPeer(pt_ctx* ctx, pt_ctx* p, int rc) {
  if (rc && p != ctx) ctx->err = "device " + std::to_string(p->cfg.device_id) + ": " + p->err;
  return rc;
}

// What one host file defines and another calls; the library exports only pt_abi.h's names
#pragma GCC visibility push(hidden)
// pt_runtime.cpp
int joinPipe(pt_ctx* ctx);     // the caller's stream waits for the last pipelined frame's running-mean update
int syncStreams(pt_ctx* ctx);  // every stream the context renders on, then its own: all work done
SceneView sceneView(const pt_ctx* ctx);  // the uploaded scene as the kernels read it (fast is set per launch)
Env envView(const pt_ctx* ctx, bool rowTable, int nt);  // the uploaded environment as the kernels read it
Share shareOf(const pt_ctx* ctx, int rank, int world);  // rank's share of a world-way screen-tile split of the image
PackParams packParams(const pt_ctx* ctx, int rank, int world);  // that share and its pixel slots
int dropMoments(pt_ctx* ctx);   // the sample moments (and what adaptive sampling decided from them) are no longer valid
int joinAdaptive(pt_ctx* ctx);  // the caller's stream waits for the last update or clear of the adaptive tile planes
void foldLaunches(pt_ctx* ctx);  // every launch's device time folded into the totals, waiting for them
// pt_scene_upload.cpp
void dropHistory(pt_ctx* ctx);  // the temporal history shows another scene or another light after an upload
void freeRefit(pt_ctx* ctx);    // pt_update_geometry's device tables and staging belong to one upload
void freeMaterialTables(pt_ctx* ctx);  // ... and so do pt_update_materials'
// pt_env.cpp
void releaseEnv(pt_ctx* ctx);  // the environment's buffers freed: an empty store and an empty view
int ensureBasicImage(pt_ctx* ctx);  // the BASIC double image, allocated and zeroed on first use
// pt_group.cpp
int createGroup(pt_ctx* ctx);    // the gather's streams, events, buffers and communicators of a device group
void destroyGroup(pt_ctx* ctx);  // ... released, and the other ranks' contexts destroyed
int groupGather(pt_ctx* ctx);    // the ranks' tiles of the frame just enqueued packed, sent and unpacked into rank 0's accumulation
int syncGroup(pt_ctx* ctx);      // every device's render stream, the gather's streams, then rank 0's stream
int joinGather(pt_ctx* ctx);     // the device group's gather of the last frame has landed in the accumulation
#pragma GCC visibility pop

