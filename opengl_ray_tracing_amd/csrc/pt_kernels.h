// pt_kernels.h -- kernel parameter blocks and launchers shared by
// the .hip files (device) and the host files of the runtime (pt_runtime.h lists them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pt {

// Structural switches retired at their shipped values (DESIGN.md "Retired build switches"): a build
// that still passes one would get the shipped code whatever value it names
#if defined(PT_FAST_TREE) || defined(PT_WIDE4) || defined(PT_FUSED_SLABS) || defined(PT_PACKETS) ||        \
    defined(PT_NT_STREAM) || defined(PT_TILE_PRIM) || defined(PT_LDS_TREE) || defined(PT_REGEN_TOP4_3) ||    \
    defined(PT_SPLIT_AUTO) || defined(PT_NO_BATCH_SPLIT_PROBE) || defined(PT_DIRECT_SOLO) ||                 \
    defined(PT_CALL_MEGAKERNEL) || defined(PT_ROW_TABLE)
#error "retired build switch: PT_FAST_TREE, PT_WIDE4, PT_FUSED_SLABS, PT_PACKETS, PT_NT_STREAM, PT_TILE_PRIM, PT_LDS_TREE, PT_REGEN_TOP4_3, PT_SPLIT_AUTO, PT_NO_BATCH_SPLIT_PROBE, PT_DIRECT_SOLO, PT_CALL_MEGAKERNEL and PT_ROW_TABLE are fixed (DESIGN.md)"
#endif

#ifndef PT_BLOCK
#define PT_BLOCK 256  // 64 and 128 measured: c2 +18 % / +8 %, c4 -6 % / -2 %
#endif
constexpr int BLOCK = PT_BLOCK;   // threads per block (256 = 4 waves of 64)
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 32
#endif
#ifndef PT_MIN_WAVES_LAMBERT
#define PT_MIN_WAVES_LAMBERT 3    // Lambert megakernel: keep 3 waves/SIMD (<= 168 VGPRs, no spills)
#endif
// Scenes whose geometry outgrows the L2s by far (> PT_WIDE_SCENE_MB of records)
// walk memory-latency bound: their Disney/MIS megakernels run the variant
// compiled for WIDE_WAVES waves per SIMD (some VGPRs spilled), which keeps more
// node fetches in flight (c5: 13.4 -> 10.5 ms; c3/c4, L2-resident: 1-5 % slower).
#ifndef PT_COST_EMA
#define PT_COST_EMA 2  // order tiles by a running estimate of their cost, this frame's weighted 2^-PT_COST_EMA (0 = off)
#endif
#ifndef PT_WIDE_SCENE_MB
#define PT_WIDE_SCENE_MB 48  // 240 B of records per triangle (pairs, geometry, shading) + 64 per node: ~200k triangles
#endif
constexpr int WIDE_WAVES = 3;
// ... and the Disney/MIS path-regeneration kernel (pt_regen.hip) compiled for 4 waves
// per SIMD (128 VGPRs, 18 spilled) is their default frame kernel: with long paths
// (c5: 16 bounces) a lane that takes a new pixel when its path ends beats the
// lock-step megakernel, whose waves last as long as their longest path (c5: 10.0
// -> 9.2 ms; on the L2-resident c4 the regen kernel is 3.6x slower)
#ifndef PT_WIDE_REGEN_WAVES
#define PT_WIDE_REGEN_WAVES 4  // MIS
#endif
// the uniform integrators' (Lambert, Disney) variant: 4 waves per SIMD since round 4's scalar pair
// test (128 VGPRs, 3 spilled; 3 waves 135 unspilled): c2 0.1938 -> 0.1884 ms per frame (5 rounds,
// profiles/r4/ab/aj_*). Before it, 3 waves (163 VGPRs) against 4 (59 spilled): 0.235 vs 0.241 ms.
#ifndef PT_WIDE_REGEN_WAVES_U
#define PT_WIDE_REGEN_WAVES_U 4
#endif
constexpr int WIDE_REGEN_WAVES = PT_WIDE_REGEN_WAVES;
constexpr int wideRegenWaves(int integrator) { return integrator == 2 ? PT_WIDE_REGEN_WAVES : PT_WIDE_REGEN_WAVES_U; }
// the MIS wide kernel on scenes that fit the L2s (c3): 3 waves per SIMD, no spills (143 VGPRs), against 4
// with 9 spilled -- c3 0.1262 -> 0.1216 ms per frame; large scenes keep 4 (c5 4.44 vs 4.79 ms at 3)
#ifndef PT_WIDE_REGEN_WAVES_SMALL
#define PT_WIDE_REGEN_WAVES_SMALL 3
#endif
#ifndef PT_MIN_WAVES
#define PT_MIN_WAVES 1            // __launch_bounds__ minimum waves per SIMD of the render kernels
#endif
// the MIS megakernel at 3 waves per SIMD (168 VGPRs; 208 uncapped, so ~30 spill): c4 0.321 ->
// 0.291 ms per frame (tools/tune.py, 3 rounds; round 3's kernel, 231 VGPRs with 142 spilled at 3
// waves, had measured no gain)
#ifndef PT_MIN_WAVES_MIS
#define PT_MIN_WAVES_MIS 3
#endif
constexpr int LDS_STACK = PT_LDS_STACK;
#ifndef PT_LDS_NODES
#define PT_LDS_NODES 128
#endif
// top-of-tree nodes (breadth-first from the root) the megakernel keeps in LDS, 64 B each
constexpr int LDS_NODES = PT_LDS_NODES;
static_assert(LDS_NODES > 0, "the frame kernels always stage the top of the tree in LDS");
#ifndef PT_SPLIT_PCT
#define PT_SPLIT_PCT 25  // megakernel: split a tile whose longest item costs more than this % of a wave's share
#endif
#ifndef PT_WAVE_TRACE
#define PT_WAVE_TRACE 0  // diagnostics build: record each megakernel wave's lifetime (tools/wave_trace.py)
#endif
#ifndef PT_PHASE_STATS
// diagnostics build (with PT_WAVE_TRACE): the regen kernel's per-wave time and lanes per phase
// (refill, walk, reference check, shading; node and leaf iterations) -- tools/wave_trace.py --phases
#define PT_PHASE_STATS 0
#endif
constexpr int PHASE_WORDS = 24;  // PT_PHASE_STATS record (pt_regen.hip)
constexpr int WAVE_TRACE_WORDS = PT_PHASE_STATS ? PHASE_WORDS : 6;  // u64 per wave in RenderParams::waveTrace
 // traversal stack entries per lane kept in LDS (4 B x 256 lanes each)
#ifndef PT_NUM_QUEUES
#define PT_NUM_QUEUES 32
#endif
// Device-scope atomics are serialised per cache line at the memory side (~88
// same-line ops/us), so every hot counter lives on its own 256-byte line.
constexpr int CTL_LINE_INTS = 64;
// records (16 bytes) of one queue's live-item segment for a launch of nFrames frames: the count's own
// line, then room for every item of the queue, a whole number of lines (RenderParams::liveItems)
constexpr int LIVE_HEAD = 16;
__host__ __device__ constexpr int liveStride(int perQueue, int nFrames) { return LIVE_HEAD + ((perQueue * nFrames + 15) & ~15); }
constexpr int NUM_QUEUES = PT_NUM_QUEUES;  // work counters, queue q owned by blocks with blockIdx % NUM_QUEUES == q
static_assert((NUM_QUEUES & (NUM_QUEUES - 1)) == 0 && NUM_QUEUES <= 64, "NUM_QUEUES: power of two <= 64");
constexpr int RAY_SHARDS = 64;     // sharded ray counters (u64, one per 256-byte line)
constexpr int RAY_SHARD_STRIDE = CTL_LINE_INTS / 2;  // in u64
// control block layout (bytes)
constexpr int MAX_SLOTS = 16;  // frames in flight the control block has queue counters for (pt_runtime.h PIPE)
constexpr size_t CTL_QUEUES = 0;  // MAX_SLOTS x NUM_QUEUES padded int counters
constexpr size_t CTL_STATS = (size_t)MAX_SLOTS * 64 * 256;            // 5 u64 cumulative fetch counters
constexpr size_t CTL_RAYS = CTL_STATS + 256;                          // RAY_SHARDS padded u64 counters
constexpr size_t CTL_BYTES = CTL_RAYS + (size_t)RAY_SHARDS * 256;
// The runtime builds and traverses its own tree (results checked against the reference's): the
// megakernel's traced rays walk it collapsed to 4-wide nodes with that tree's top 64 nodes in LDS
// (pt_trace.h traceRay4), its camera rays keep their bins and the binary tree's wave packets
// (tracePacket), whose slab tests are fused (visitNodeF).
#ifndef PT_ACCEL_LEAF
#define PT_ACCEL_LEAF 4  // most triangles per leaf of the runtime's tree
#endif
constexpr int PKT_DEPTH = 128;    // camera-ray packet stack entries per wave (LDS); deeper trees trace per ray
constexpr int PAIR_F4 = 7;        // float4 per pair record (26 floats: p1, p2, p3, Ng, w of two triangles)
constexpr int HIT_F4 = 4;         // float4 per hit record (SceneView::hitRec)
constexpr int MAT_F4 = 5;         // float4 per material (SceneView::mats)
constexpr int W4_F4 = 8;          // float4 per 4-wide node as built (collapseWide4Device, encodeWide4), one 128-byte line
constexpr int LEAF_CNT_BITS = 5;  // leaf refs: ~(start << 5 | (count - 1)), count <= 32
constexpr int REF_NONE = (int)0x80000000;
constexpr int MAX_LEAF = 1 << LEAF_CNT_BITS;
constexpr int MAX_TRIS = (1 << (31 - LEAF_CNT_BITS)) - 1;

// Device-resident scene (relaid out at upload, see pt_scene_prep.cpp)
struct SceneView {
  const float4* geo;   // 4 float4 per triangle: (p1, w=dot(Ng,p1)), (p2, 0), (p3, 0), (Ng, 0)
  const float4* pairs; // PAIR_F4 float4 per triangle i: triangles i and i+1 component-interleaved (pt_trace.h pairTest)
  // Shading data of a hit, read once per closest hit (finishHit): per triangle one
  // 64-byte record {n1.xyz, n2.x}, {n2.yz, n3.xy}, {n3.z, material id, -, -} (the
  // Triangle_encoded normals, floats 9..17), and the scene's distinct materials,
  // MAT_F4 float4 each laid out as Triangle_encoded floats 16..35 (emissive at
  // floats 18..20, IS:207-232). 64 + ~0 bytes per triangle instead of 144.
  const float4* hitRec;
  const float4* mats;
  int nMats;           // materials in mats
  const float4* bvh;   // 4 float4 per device node id (pt_scene_prep.cpp: top of the tree first, breadth-first)
  int nTop;            // device ids [0, nTop) are the top of the tree, staged in LDS by the megakernel
  int rootRef;         // encoded reference to node 1
  int nTri;
  // The runtime's own tree over the same triangles (pt_scene_prep.cpp prepareAccel;
  // pt_trace.h "Reference-exact results through the runtime's tree"): wide
  // nodes with conservative boxes, pair records in its leaf order, and for
  // every position the uploaded triangle index. fast = 0: not used this launch.
  int fast;
  const float4* fbvh;
  const float4* fpairs;
  const int* fastTri;
  int fRoot;
  int fnTop;  // (read by the fetch-counting megakernel's staging alone, pt_kernels.hip renderKernel)
  // the same tree collapsed to 4-wide nodes (pt_scene_prep.cpp encodeWide4; pt_trace.h
  // traceRay4): W4_F4 float4 per node, breadth-first ids, leaves as in fbvh; null = none
  const float4* fbvh4;
  int f4Root, f4nTop;
  // reference facts: each triangle's reference leaf's box (lo, hi; lo.w = the leaf's node id as
  // int bits, -1 = in no leaf), every reference node's parent and box (lo, hi)
  const int* refParent;
  const float4* refBox;
  const float4* leafBox;
};

// The origin domain of the runtime tree (derived where its boxes' widening is set: pt_scene_prep.cpp
// prepareAccel): a ray is in domain iff every |origin coordinate| <= PT_ORIGIN_K x the scene scale, the
// largest coordinate magnitude of the tree's root box. Out of it -- a NaN or an infinite coordinate fails
// the comparisons too -- the fused slab tests no longer hold their rounding below the widening, so the ray
// never enters the runtime tree: it takes the reference-order walk of the uploaded tree, which is exact
// for every origin. limit = PT_ORIGIN_K x scale, computed once per runtime tree (pt_ctx::originLimit).
constexpr float PT_ORIGIN_K = 32.0f;
__host__ __device__ inline bool originInDomain(float ox, float oy, float oz, float limit) {
  return fabsf(ox) <= limit && fabsf(oy) <= limit && fabsf(oz) <= limit;
}

// HDR environment (hdrMap + hdrCache textures, IS main.cpp:843-853), float4 texels
// Render layout: one 16-byte texel serves hdrColor and hdrPdf of a direction
// together (every MIS lookup pairs them), so a miss costs one line, not two.
struct Env {
  const float4* hdr;    // w x h: (r, g, b, calculateHdrCache pdf) (row 0 = first scanline); null = black
  const float2* cache;  // calculateHdrCache sample table (x, y); null exactly when hdr is null
  // The same texels in half the bytes, used when non-null (pt_env.cpp envOne builds them when
  // every texel round-trips bit for bit, pt_envcache.hip envCompactKernel): hdr8 = {r | g << 8 |
  // b << 16 | E << 24, pdf bits}, each channel m * 2^(E - 136) -- the Radiance RGBE form the
  // reference's decoder expands (hdrloader.cpp:99-104) -- and cache4 = x | y << 16, the sample
  // table's float(x) / w and float(y) / h (IS main.cpp:630-631)
  const uint2* hdr8;
  const uint32_t* cache4;
  // The sample table by rows, used when non-null: calculateHdrCache's entry (row i, column j) is
  // (x(i) / w, y(x(i), j) / h) -- x from the marginal CDF at xi_1 = i / h, y from column x's
  // conditional CDF at xi_2 = j / w (IS main.cpp:621-634) -- so all rows of one x are equal.
  // cacheRow[i] = x(i) | (its distinct row's id) << 16, cacheY[id * w + j] = y; c4's 8 MB of uniformly
  // read 4-byte entries become 639 distinct rows of 2-byte ones (2.6 MB) and a 4 KB row table
  const uint32_t* cacheRow;
  const unsigned short* cacheY;
  // With the compact table: SampleHdr's (sin, cos) of theta for each y integer 0..h, then of phi
  // for each x integer 0..w (launchEnvTrig: the device functions of the same floats), null = computed
  const float2* trig;
  // With the compact texels too: per sample-table entry (y, x) (index y * (w + 1) + x, x <= w, y <= h)
  // the light sample's hdrColor and hdrPdf (IS:647-666) of SampleHdr's direction: {the texel's RGBE,
  // the pdf's bits} (launchEnvLight: the device functions of the same floats), null = computed
  const uint2* light;
  int w, h, res;        // res = hdrResolution
  // texels read as streaming (non-temporal) loads, so they leave L2 before the scene's lines: on
  // scenes larger than L2 (c5 4.15 vs 4.32 ms per frame with plain loads); on small scenes plain
  // loads let neighbouring rays share env lines (c2 0.1722 -> 0.1684, c3 0.1097 -> 0.1068, c4
  // 0.2969 -> 0.290 ms)
  int nt;
};

// One frame of a launch as a work item sees it: its sample index (RNG seeds, Sobol
// index) and its colour buffer (null: the running mean is updated in place).
constexpr int COL_F = 3;  // floats per pixel of a pipelined frame's colour buffer (r, g, b)
struct FrameRef {
  float* col;  // COL_F floats per pixel of the share
  uint32_t sampleIndex;
};

// A context's screen-tile share of the image: shard tiles (shardSize x shardSize pixels, row-major ids
// over the image, shardsX per row) g with g % world == rank, in id order. pt_frame.h holds everything
// derived from it: the share's wave tiles, its slots (the packed order of pt_pack_owned) and their pixels.
struct Share {
  int width, height;
  int shardSize;  // shard tile edge (multiple of 8)
  int shardsX;    // shard tiles per row
  int rank, world;
};

struct RenderParams {
  SceneView scene;
  Env env;
  int width, height;    // the six fields of the context's Share (pt_frame.h shareOf / setShare) keep their places
                        // in the block: the frame kernels' scalar register use follows its layout
  uint32_t frameCounter;  // running-mean count: weight 1/(frameCounter+1) (IS:868-871)
  uint32_t sampleIndex;   // RNG / Sobol sample index: frameCounter*sample_world + sample_rank
  int maxBounce;
  float eye[3];
  float cam[16];
  float4* accum;
  // Pipelined frames (pt_runtime.h "frames in flight"): non-null = write each pixel's
  // sample colour here (float4, w unused) and leave the running mean to mixKernel, which
  // runs in frame order; null = mix into accum in place (IS:868-871)
  float* col;  // COL_F floats per slot of the share
  // A batch of nFrames consecutive frames of one camera in this launch (pt_render_frames_async):
  // frame f draws sample index sampleIndex + f * sampleStride and writes its colours to
  // col + f * colStride and its camera-ray results to primHit + f * colStride, each indexed by the
  // pixel's slot in this context's screen-tile share (pt_frame.h slotOf: the packed order of
  // pt_pack_owned; colStride = slots(share)), so a 1/N share's buffers are 1/N of a frame. Work
  // item k of the launch is item k / nFrames of frame k % nFrames, so the frames of one tile
  // run side by side (the same camera rays, the same nodes). nFrames 1: a single frame.
  int nFrames;
  uint32_t sampleStride;
  size_t colStride;
  // camera-ray bins (pt_primary.hip): per 8x8 tile of the whole image, binStart[t] ..
  // binStart[t+1] index binTris; null = every camera ray walks the BVH
  const int* binStart;
  const int* binTris;
  // per bin entry: its triangle's geometry record (4 float4) and reference leaf box (2 float4),
  // gathered at bin build so the camera-ray pass stages a tile's bin in one round trip
  const float4* binGeo;
  const float4* binBox;
  int binTilesX, binTilesY;
  // camera-ray pass (primaryKernel): per pixel (py * width + px) the camera ray's result,
  // {tri, t bits}: tri >= 0 a hit, PRIM_MISS (finished: sky colour written), PRIM_RETRACE
  // (a tie or an unreachable winner: the megakernel traces it in the reference order),
  // PRIM_TILE (the tile's bin is over PT_BIN_CAP: the megakernel traces the tile's
  // packet); null = the megakernel traces its camera rays itself
  int2* primHit;
  // ... compacted per 8x8 wave tile (round 6): tile w of frame f has a 64-bit mask of the slots that
  // need a path (primMask[f * numItems + w]: not sky, inside the image) and their results in slot
  // order at primHit + (f * numItems + w) * 64 (primOfSlot); sky slots cost no bytes
  unsigned long long* primMask;
  // ... and, for the regen kernels, each work queue's live items (liveListKernel, after the pass):
  // queue q's claims in claim order without those whose mask is 0 (all sky, or outside the image).
  // Queue q's segment starts at liveItems + q * liveStride(perQueue, nFrames): one 256-byte line
  // whose first int is the number of live items, then the records {tile, frame, mask lo, mask hi};
  // null = every item is claimed (large scenes, pt_runtime.cpp; no pass)
  uint4* liveItems;
  int zeroQueue;  // the camera-ray pass zeroes `queue` for the frame kernel after it (no memset)
  int* queue;           // NUM_QUEUES counters (stride CTL_LINE_INTS), zeroed before each launch
  int perQueue;         // items per queue (band), claimed once per frame of the launch
  int numItems;         // 8x8 wave tiles owned by this rank (slots(share) / 64)
  int shardSize;        // shard tile edge (multiple of 8)
  int shardTiles;       // (shardSize/8)^2, the divisor of the kernels' tile -> shard tile step
  int shardsX;          // shard tiles per row
  int rank, world;
  int* ovf;             // traversal stack overflow (per thread ovfDepth ints), may be null
  int ovfDepth;
  int packets;          // camera rays traced as wave packets (tree depth fits PKT_DEPTH)
  unsigned long long* stats;  // [rays, nodes, tris, mats, texels]
  unsigned long long* rayShards;  // RAY_SHARDS ray counters (stride RAY_SHARD_STRIDE)
  const int* tileOrder; // per-band work items (null = one per tile, in id order), then NUM_QUEUES item
                        // counts; see TileCursor / reorderKernel
  int orderCap;         // entries per band in tileOrder
  int* tileCost;        // per tile: summed cost of its items this frame (shader cycles), null = not recorded
  int* tileCostMax;     // per tile: its longest item this frame
  unsigned long long* waveTrace;  // PT_WAVE_TRACE builds only: WAVE_TRACE_WORDS u64 per wave (pt_runtime.cpp, tools/wave_trace.py)
  // PT_FLAG_ADAPTIVE (pt_adaptive.hip): per 8x8 tile of the whole image (ty * tilesX + tx, tilesX =
  // (width + 7) / 8) the frame count at which the tile retired, 0 = active; null without the flag. Only
  // the camera-ray pass reads it: a retired tile gets mask 0, so no frame kernel touches it
  const uint32_t* retiredAt;
};

// The ray queries on device memory (pt_query.hip queryKernel; pt_abi.h pt_trace_closest_device,
// pt_trace_occluded_device): ray k's closest hit below tmax[k], or whether it has one
struct QueryParams {
  SceneView scene;
  const float* rays;   // n x 6 (origin, direction)
  const float* tmax;   // n bounds; null: none (PT_INF)
  int n;
  float* t;            // closest: n distances (a miss PT_INF) ...
  int* tri;            // ... and uploaded triangle indices (a miss -1)
  uint8_t* occ;        // occluded: n bytes, 0 / 1
  int* ovf;            // the queries' own traversal stack overflow (per thread ovfDepth ints), may be null
  int ovfDepth;
  float originLimit;   // the runtime tree's origin domain (originInDomain): rays from beyond it walk the uploaded tree
};

// Radiance along caller-supplied rays (pt_radiance.hip radianceKernel; pt_abi.h pt_radiance_device): one
// sample of the context's integrator along ray k, seeded as pixel ids[k] of sample sampleIndex
struct RadianceParams {
  SceneView scene;
  Env env;
  const float* rays;   // n x 6 (origin, direction)
  const int* ids;      // n x 2 (px, py); null: (k & 4095, k >> 12)
  int n;
  uint32_t sampleIndex;
  int maxBounce;
  float4* out;         // n x (r, g, b, t); a miss (sky, PT_INF)
  int* ovf;            // the queries' traversal stack overflow (per thread ovfDepth ints), may be null
  int ovfDepth;
  float originLimit;   // as QueryParams': the caller's ray alone is checked, a bounce starts on the scene
};
// waves per SIMD the radiance kernel is compiled for, per integrator
#ifndef PT_RADIANCE_WAVES_LAMBERT
#define PT_RADIANCE_WAVES_LAMBERT 4
#endif
#ifndef PT_RADIANCE_WAVES_DISNEY
#define PT_RADIANCE_WAVES_DISNEY 3
#endif
#ifndef PT_RADIANCE_WAVES_MIS
#define PT_RADIANCE_WAVES_MIS 3
#endif
hipError_t launchRadiance(const RadianceParams& p, int integrator, int grid, hipStream_t s, bool cull);
// nSamples samples per ray folded into a running mean and the luminance moments (pt_radiance_mean.hip
// radianceMeanKernel; pt_abi.h pt_radiance_mean_device): sample j of ray k is radianceKernel's for sample
// index firstSample + j, the fold pt_display.hip mixFrames'
struct RadianceMeanParams {
  SceneView scene;
  Env env;
  const float* rays;   // n x 6, or nSamples x n x 6 (perSample): sample j's ray k at rays + 6 * (j * n + k)
  const int* ids;      // n x 2 (px, py); null: (k & 4095, k >> 12)
  int n;
  uint32_t firstSample;
  int nSamples;        // >= 1, firstSample + nSamples <= 2^32 - 1
  int perSample;
  int maxBounce;
  float4* mean;        // n x (r, g, b, t of the last sample's ray); read when firstSample != 0
  float2* moments;     // n x (m1, m2), may be null; read when firstSample != 0
  int* ovf;            // the queries' traversal stack overflow (per thread ovfDepth ints), may be null
  int ovfDepth;
  float originLimit;   // as RadianceParams'
};
hipError_t launchRadianceMean(const RadianceMeanParams& p, int integrator, int grid, hipStream_t s, bool cull);
// The frame kernels' camera rays of one sample (pt_frame.h cameraRay) for every pixel of a width x height
// image: ray py * width + px = (eye, direction) into rays (6 floats each), (px, py) into ids (may be null)
struct CameraRaysParams {
  int width, height;
  uint32_t sampleIndex;
  float eye[3];
  float cam[16];
  float* rays;
  int* ids;
};
hipError_t launchCameraRays(const CameraRaysParams& p, hipStream_t s);

// BasicRayTracingWithC++ (pt_basic.hip basicKernel): one sample k of every pixel
constexpr int BASIC_MAX_DEPTH = 31;  // pathTracing vertices kept for the fold (the reference's cutoff is 8)
struct BasicParams {
  const double* shapes;         // nShapes x PT_SHAPE_DOUBLES
  int nShapes;
  int width, height;
  uint32_t sample, seed;        // k, and the counter RNG's run seed
  int maxDepth;
  int reset;                    // frameCounter == 0: this sample starts the image
  float brightness;             // BRIGHTNESS (B:20) as glm's operator*= casts it
  float4* accum;                // the image as f32 (pt_download_accum)
  double* image;                // the reference's double image, width x height x 3 (B:356)
  const double* stream;         // replayed randf() stream (nullable: counter RNG)
  const long long* offsets;     // replay: start of each sample's draws, (k * height + i) * width + j
  long long streamN, nOffsets;
  unsigned long long* stats;    // ray counter
  unsigned long long* overruns; // replay: pixel samples that read past their draws
};

struct PackParams {
  Share share;
  long count;  // slots(share)
};
// rank 0's unpack of ranks 1..world-1's packed buffers in one launch (pt_display_unpack: RGB8
// display values; pt_unpack_ranks: f32 running means); null buffers are skipped; base's rank /
// count are per rank
constexpr int DISPLAY_MAX_WORLD = 16;
struct RanksUnpack {
  PackParams base;
  const void* src[DISPLAY_MAX_WORLD];
  long count[DISPLAY_MAX_WORLD];
};

// camera-ray bins of one camera (pt_primary.hip), device buffers owned by the context
#ifndef PT_BIN_CAP
#define PT_BIN_CAP 32  // a tile whose bin holds more triangles traces its camera rays through the BVH
#endif
#ifndef PT_PASS_BIN_CAP
#define PT_PASS_BIN_CAP 64  // the camera-ray pass (primaryKernel), staged per one-wave block: c5 32 6.84, 64 6.77, 128 6.79, 256 7.08 ms
#endif
#ifndef PT_BINS
#define PT_BINS 1      // 0: no camera-ray bins
#endif
struct PrimaryBins {
  int4* rect = nullptr;      // per triangle: its tile rectangle
  int* triCount = nullptr;   // per triangle: its tiles (+1: the scan total)
  int* triOffset = nullptr;
  int* tileCount = nullptr;  // per tile: its triangles, then the fill cursors
  int* binStart = nullptr;   // per tile (+1)
  int* binTris = nullptr;
  float4* binGeo = nullptr;  // per entry: geo[4 tri .. 4 tri + 3] (RenderParams::binGeo)
  float4* binBox = nullptr;  // per entry: leafBox[2 tri], [2 tri + 1]
  void* tmp = nullptr;       // hipcub scan scratch
  // the pass tiles of the context's share (buildPassList): the share's wave tiles whose image tile has a
  // non-empty bin, ascending, then their number at passList[waveTiles(share)]
  int* passList = nullptr;
  size_t rectCap = 0, triCountCap = 0, triOffsetCap = 0, tileCountCap = 0, binStartCap = 0, binTrisCap = 0,
         binGeoCap = 0, binBoxCap = 0, tmpBytes = 0, passListCap = 0;
  int tilesX = 0, tilesY = 0, entries = 0;
  int passCount = 0;         // the list's length, read back at its build
};
hipError_t buildPrimaryBins(const float eye[3], const float cam[16], int width, int height, const float4* geo,
                            const float4* leafBox, int nTri, PrimaryBins& b, hipStream_t s);
// b's pass tiles of `share` (after buildPrimaryBins, on its stream; one more host sync for the count)
hipError_t buildPassList(const Share& share, PrimaryBins& b, hipStream_t s);
void freePrimaryBins(PrimaryBins& b);

// The runtime's own tree built on the device (pt_build.hip): a binned-SAH tree
// over the triangles of geo (SceneView::geo layout), its wide records with
// every box widened by inflate of its own magnitude plus inflateRelAbs x the
// scene's largest coordinate (pt_scene_prep.cpp encodeWideTree), the pair records
// in its leaf order and that order. Device buffers owned by the caller
// (freeAccelBuild); the stream is synchronised on return.
struct BuildNode {  // 64 B, breadth-first ids (root 0)
  float4 lo;        // triangle box lo; w: first position (int bits)
  float4 hi;        // triangle box hi; w: triangle count (int bits)
  float4 clo;       // centroid bounds lo; w: left child id (int bits, -1 = leaf)
  float4 chi;       // centroid bounds hi; w: right child id
};
struct AccelBuild {
  float4* bvh = nullptr;    // nDev wide records (4 float4 each)
  float4* pairs = nullptr;  // nTri pair records (PAIR_F4 float4 each), leaf order
  int* order = nullptr;     // position -> uploaded triangle index
  BuildNode* nodes = nullptr;  // the nNodes build nodes (leaves: count <= leafSize)
  int rootRef = REF_NONE, nDev = 0, depth = 0, nNodes = 0;
};
hipError_t buildAccelDevice(const float4* geo, int nTri, int leafSize, float inflate, float inflateRelAbs,
                            AccelBuild& out, hipStream_t s);
void freeAccelBuild(AccelBuild& a);
// the build nodes collapsed to 4-wide records (SceneView::fbvh4, pt_scene_prep.cpp encodeWide4's
// layout, ids and widening) on the device; *out allocated here (W4_F4 float4 per wide node)
// *scale: the scene scale the widening used, the root box's largest coordinate magnitude
hipError_t collapseWide4Device(const BuildNode* nodes, int nNodes, int leafSize, float inflate, float inflateRelAbs,
                               float4** out, int* rootRef, int* nDev, int* depth, float* scale, hipStream_t s);

// New vertex positions in place (pt_refit.hip, pt_abi.h pt_update_geometry): the geometry, pair and
// shading records rewritten from the caller's vertex records, the uploaded tree's boxes refitted
// bottom-up into refBox, and the uploaded tree's wide records and the triangles' leaf boxes rewritten
// from them. The topology comes from the upload (pt_scene_upload.cpp makeRefit): the tables below are
// device memory, made at the first update of a scene.
struct RefitTables {
  int2* topo = nullptr;       // per reference node: internal (left, right), 0 = absent; leaf (first triangle, -count)
  int* byHeight = nullptr;    // the reachable nodes, leaves (height 0) first, then by height
  int* heightStart = nullptr; // heights + 1 offsets into byHeight
  int2* devKids = nullptr;    // per device wide node: its children's reference ids (0 = absent)
  int heights = 0;            // heights of the reachable tree (a root leaf: 1)
  int tailFrom = 0;           // the one-block tail walks heights tailFrom .. heights - 1
  bool ready = false;
};
constexpr int REFIT_TAIL = 1024;  // threads of the tail's block: most nodes of a height it takes over from the launches
struct RefitParams {
  const float* verts;  // record i at verts + i * stride: p1 p2 p3 n1 n2 n3
  int stride;
  int nTri, nDevNodes;
  float4* geo;
  float4* pairs;
  float4* hitRec;
  float4* bvh;
  float4* refBox;
  float4* leafBox;     // null: the scene has no runtime tree
};
// hostStart: the tables' heightStart on the host (heights + 1 entries); ev (nullable): 4 events recorded
// before the records, the refit, the re-encode and after it
hipError_t launchRefit(const RefitParams& p, const RefitTables& t, const int* hostStart, hipEvent_t* ev, hipStream_t s);

// New materials in place (pt_materials.hip; pt_abi.h pt_update_materials): the table of distinct
// materials and every triangle's id rewritten from the caller's material records. The tables below are
// device memory, made at the first material update of a scene (pt_scene_upload.cpp makeMaterialTables).
constexpr int MAT_KEY = 18;  // words of a material key: Triangle_encoded floats 18..35
struct MaterialTables {
  int* slots = nullptr;    // nSlots triangle indices, -1 = empty: the open-addressed table of the insert
  int* slotOf = nullptr;   // per triangle: the slot its key ended in
  int* flag = nullptr;     // per triangle: 1 = the first appearance of its key
  int* rank = nullptr;     // per triangle: first appearances before it (the exclusive scan of flag)
  int* count = nullptr;    // the number of distinct keys
  void* scanTmp = nullptr; // hipcub scan scratch
  size_t scanBytes = 0;
  int nSlots = 0;          // a power of two >= 2 * nTri (materialSlots)
  bool ready = false;
};
struct MaterialParams {
  const float* mats;  // record i: the MAT_KEY floats at mats + i * stride
  int stride;
  int nTri;
  float4* hitRec;     // [i][2].y takes triangle i's id; nothing else of the record is written
  float4* table;      // room for nTri entries of MAT_F4 float4
};
int materialSlots(int nTri);
hipError_t materialScanBytes(int nTri, size_t* bytes);
// ev (nullable): 4 events recorded before the insert, the flags and scan, the scatter and after it
hipError_t launchMaterials(const MaterialParams& p, const MaterialTables& t, hipEvent_t* ev, hipStream_t s);

// calculateHdrCache on the device (pt_envcache.hip); scratch: 2*w*h + 2*w + 1 floats
hipError_t launchHdrCache(const float* hdr, int w, int h, float4* cache, float* scratch, hipStream_t s);
// hdr[k].w = cache[k].z, samp[k] = cache[k].xy (the Env render layout)
hipError_t launchEnvCompact(const float4* hdr, const float2* cache, int w, int h, uint2* hdr8, uint32_t* cache4,
                            int* bad, hipStream_t s);
hipError_t launchEnvPack(float4* hdr, const float4* cache, float2* samp, int n, hipStream_t s);
// Env::trig: (h + 1) + (w + 1) entries
hipError_t launchEnvTrig(float2* trig, int w, int h, hipStream_t s);
// Env::light: (w + 1) * (h + 1) entries, from e's compact texels and trig table
hipError_t launchEnvLight(const Env& e, uint2* light, hipStream_t s);
hipError_t launchRender(const RenderParams& p, int integrator, int grid, hipStream_t s, bool cull, bool count,
                        bool wide = false);
// tile order of the next frame: each queue band's groups of `group` consecutive
// tiles sorted by this frame's summed cost, descending (tiles inside a group keep
// their order, which keeps neighbouring tiles together for the caches)
constexpr int REORDER_MAX = 4096;  // most groups per band the one-block LDS sort handles
// order: NUM_QUEUES * orderCap items, then NUM_QUEUES item counts; cost / costMax are read
// and zeroed; splitLg (one per tile) is the split state carried from frame to frame
hipError_t launchReorder(int* cost, int* costMax, int* splitLg, int* ema, int* order, int perQueue, int orderCap,
                         int numItems, int group, int numWaves, int splitPct, hipStream_t s);
hipError_t renderBlocksPerCU(int integrator, bool cull, bool count, bool wide, int* nb);
// the camera-ray pass: one wave per 8x8 tile of the rank's tiles, results in p.primHit
constexpr int PRIM_MISS = -1, PRIM_RETRACE = -2, PRIM_TILE = -3;
// passList (PrimaryBins::passList, passCount > 0 entries): the pass over those tiles only -- a pipelined
// launch, whose running-mean update takes the other tiles' samples (SkyTiles); null: every tile of the share
hipError_t launchPrimary(const RenderParams& p, const int* passList, int passCount, hipStream_t s);
// the live items of every work queue from the pass's tile masks (p.liveItems), for the regen kernels
hipError_t launchLiveList(const RenderParams& p, hipStream_t s);
// the path-regeneration kernel (pt_regen.hip): the variant and launch shape of a frame
struct RegenVariant {     // one instantiation of regenKernel and what the host needs to know of it
  const void* fn = nullptr;
  int waves = 0;          // waves per SIMD it is compiled for (0: the integrator's default)
  int block = BLOCK;      // threads per block
  bool lists = true;      // it claims from live-item lists after a camera-ray pass
  int top4 = 0;           // 4-wide nodes it stages in LDS (PT_REGEN_TOP4)
};
struct RegenShape {
  bool wide = false;      // the large-scene variant (WIDE_REGEN_WAVES, 4-wide walk, dynamic ray fetch)
  bool fullTree = false;  // ... with the whole 4-wide tree in LDS (small trees, uniform integrators)
  bool small = false;     // the MIS variant at PT_WIDE_REGEN_WAVES_SMALL waves per SIMD (scenes that fit the L2s)
  RegenVariant v;         // the kernel these choose (pt_regen.hip regenVariant)
  int blocksPerCU = 0;    // resident blocks per CU
  size_t dynLds = 0;      // dynamic LDS bytes per block (the tree)
};
// f4nDev: nodes of the 4-wide runtime tree the frame walks (0: it walks none)
// smallScene: the scene's records fit the L2s (not a PT_WIDE_SCENE_MB scene)
hipError_t regenShape(int integrator, bool cull, bool wide, int f4nDev, bool smallScene, RegenShape* out);
hipError_t launchRegen(const RenderParams& p, int integrator, int grid, hipStream_t s, bool cull, const RegenShape& r);
bool regenTakesLists(int integrator, const RegenShape& r);  // the variant claims from live-item lists after a pass
int regenLdsStack();
int regenTop4(const RegenShape& r, int integrator);  // 4-wide nodes the wide regen kernel stages in LDS
// occluded: the any-hit query into p.occ, else the closest hit into p.t / p.tri
hipError_t launchQuery(const QueryParams& p, int grid, hipStream_t s, bool occluded, bool cull);
// Guide buffers (pt_guides.hip): the camera's first hit of every pixel centre, one lane per pixel,
// one wave per 8x8 tile (a grid-stride loop over the tiles), three float4 planes
struct GuideParams {
  SceneView scene;
  int width, height;
  float eye[3];
  float cam[16];
  float4* posT;    // (P, t); a miss (0, 0, 0, PT_INF)
  float4* nrmTri;  // (N, triangle index bits); a miss (0, 0, 0, bits(-1))
  float4* albedo;  // (baseColor, 1); a miss 0
  int* ovf;        // traversal stack overflow (per thread ovfDepth ints), may be null
  int ovfDepth;
};
hipError_t launchGuides(const GuideParams& p, int grid, hipStream_t s, bool cull);
// One pass of an a-trous filter (pt_atrous.h): what the two filters' passes share
struct AtrousCommon {
  int width, height;
  int stride;                // 2^pass
  const float4* in;
  float4* out;
  const float4* posT;
  const float4* nrmTri;
  const float4* albedo;
  float sigmaZ;              // <= 0: term off
  float albDen;              // sigma_a^2
  int albOn;
  int normalLog2;            // -1: term off
  float limit;
};
// The edge-avoiding a-trous filter (pt_denoise.hip), one launch per pass. Every pass reads its
// input colour `in` and that colour tone-mapped `tmIn` (both float4 planes), and writes `out` and,
// for the next pass, tm(out) to `tmOut` (null on the last pass); launchAtrousTm writes the first
// pass's tm plane from the accumulation.
struct AtrousParams : AtrousCommon {
  const float4* tmIn;
  float4* tmOut;
  float colDen;              // sigma_c_i^2
  int colOn;
};
constexpr int ATROUS_TILE = 16;     // a block's 16 x 16 output pixels
constexpr int ATROUS_LDS_STRIDE = 2;  // passes of stride <= this stage their tile + halo in LDS
hipError_t launchAtrousTm(const float4* in, float4* tm, int n, float limit, hipStream_t s);
hipError_t launchAtrous(const AtrousParams& p, hipStream_t s);
// The variance-guided a-trous filter (pt_variance.hip, pt_abi.h pt_denoise_var). launchVarLum writes
// l = lum(tm(in)) per pixel; launchVarInit (step A) the initial variance, to var0 and, beside l, to the
// first pass's (l, v) plane: from the sample moments (non-null) or from l's 7 x 7 window.
struct VarInitParams {
  int width, height;
  const float4* in;
  const float4* nrmTri;
  const float2* moments;     // (m1, m2) of the sample luminance; null: the spatial estimate
  const float* lum;
  float* var0;
  float2* lv;
  float kf;                  // (float)frames the moments hold
  float limit;
};
// One launch per pass: reads the colour `in` and its (l, v) plane `lvIn`, writes `out` and, for the
// next pass, (lum(tm(out)), v_out) to `lvOut` (null on the last pass).
struct AtrousVarParams : AtrousCommon {
  const float2* lvIn;
  float2* lvOut;
  float sigmaL;              // <= 0: term off
};
hipError_t launchVarLum(const float4* in, float* lum, int n, float limit, hipStream_t s);
hipError_t launchVarInit(const VarInitParams& p, hipStream_t s);
hipError_t launchAtrousVar(const AtrousVarParams& p, hipStream_t s);
// The temporal resolve (pt_temporal.hip): the running mean `accum` blended, weighted by sample count,
// with the previous camera's resolved image `hist` fetched through the current first-hit positions
// (pt_abi.h pt_temporal_resolve). hist null: no history (out = accum's rgb, count `frames`).
struct TemporalParams {
  int width, height;
  const float4* accum;       // the running mean of the current camera
  const float4* posT;        // the current guides
  const float4* nrmTri;
  const float4* hist;        // the history's resolved image (rgb, sample count), may be null
  const float4* histPosT;    // and the guides it was committed with
  const float4* histNrmTri;
  float4* out;
  float eye[3];              // the history camera: eye and the rotation's first three columns
  float c0[3], c1[3], c2[3];
  float sigmaZ, normalCos, maxHistory;
  float frames;              // (float)frames of the accumulation
};
constexpr int TEMPORAL_TILE = 16;  // a block's 16 x 16 pixels, each wave an 8 x 8 quadrant
hipError_t launchTemporal(const TemporalParams& p, hipStream_t s);
hipError_t launchBasic(const BasicParams& p, hipStream_t s);
// BASIC checkpoints: the double image from the f32 sums (widened), or the f32 sums from the double image
hipError_t launchBasicWiden(const float4* accum, double* image, long n, hipStream_t s);
hipError_t launchBasicNarrow(const double* image, float4* accum, long n, hipStream_t s);
hipError_t launchTonemap(const float4* accum, float* rgb, int n, float limit, float gamma, hipStream_t s);
// PACK_F floats (r, g, b) per packed slot
constexpr int PACK_F = 3;
hipError_t launchPack(const PackParams& p, const float4* accum, float* packed, hipStream_t s);
hipError_t launchFmath(int fn, const float* x, const float* y, int n, float* out, hipStream_t s);
hipError_t launchSphTexel(int W, int H, const float* dirs, int n, int* texel, int* texelExact, hipStream_t s);
hipError_t launchDisplayPack(const PackParams& p, const float4* accum, float limit, float gamma, uint8_t* packed,
                             hipStream_t s);
hipError_t launchDisplayOwn(const PackParams& p, const float4* accum, float limit, float gamma, uchar4* image,
                            hipStream_t s);
hipError_t launchDisplayUnpack(const RanksUnpack& d, int world, uchar4* image, hipStream_t s);
hipError_t launchUnpackRanks(const RanksUnpack& d, int world, float4* accum, hipStream_t s);
hipError_t launchUnpack(const PackParams& p, float4* accum, const float* packed, hipStream_t s);
// The gather of a PT_FLAG_SHARE_MOMENTS split (pt_pack_owned_stats, pt_unpack_ranks_stats): launchPack and
// launchUnpackRanks with the pixel's moments behind its colour, PACK_STATS_F floats (r, g, b, m1, m2) per slot
constexpr int PACK_STATS_F = 5;
hipError_t launchPackStats(const PackParams& p, const float4* accum, const float2* moments, float* packed, hipStream_t s);
hipError_t launchUnpackRanksStats(const RanksUnpack& d, int world, float4* accum, float2* moments, hipStream_t s);
// The samples the running-mean update takes itself: in a pipelined launch a tile whose camera-ray bin is
// empty -- no camera ray of it, whatever its jitter, hits anything -- is not given to the camera-ray pass;
// the update computes sampleHdr(env, cameraRay(...)) of each of its pixels and frames where it would load
// the colour buffer (pt_display.hip mixFrames), and counts those rays. By value: the update runs on the
// caller's stream after the slot's parameter block may have been reused. binStart null: no such tiles
// (a launch without bins or without a pass; every sample comes from the colour buffer).
struct SkyTiles {
  const int* binStart;   // RenderParams::binStart of the launch
  int binTilesX;
  uint32_t sampleIndex;  // of the launch's first frame, and the step to the next (RenderParams)
  uint32_t sampleStride;
  float cam[16];
  Env env;               // the launch's view of the environment (its nt / row-table setting included)
  unsigned long long* rayShards;
};
// the running-mean updates of nFrames pipelined frames over the rank's owned pixels (PackParams
// mapping), in frame order: for f = 0 .. nFrames-1, accum = mix(accum, col + f * colStride,
// 1 / (frameCounter + f + 1)) (IS:868-871, pass2.fsh:15) -- each pixel read and written once
hipError_t launchMix(const PackParams& p, float4* accum, const float* col, size_t colStride, int nFrames,
                     uint32_t frameCounter, const SkyTiles& sky, hipStream_t s);
// launchMix of a PT_FLAG_MOMENTS context (pt_display.hip mixFrames<true>): the same update of accum, and with the same
// weights the running means (m1, m2) of each sample's luminance l and of l * l in `moments`
hipError_t launchMixMoments(const PackParams& p, float4* accum, float2* moments, const float* col, size_t colStride,
                            int nFrames, uint32_t frameCounter, const SkyTiles& sky, hipStream_t s);
// launchMixMoments of a PT_FLAG_ADAPTIVE context (mixFrames' third case): a pixel whose 8x8 tile is
// retired (retiredAt, RenderParams::retiredAt's plane) is left alone, before any of its loads
hipError_t launchMixAdaptive(const PackParams& p, float4* accum, float2* moments, const float* col, size_t colStride,
                             int nFrames, uint32_t frameCounter, const uint32_t* retiredAt, const SkyTiles& sky,
                             hipStream_t s);
// Adaptive sampling's decision (pt_adaptive.hip tileErrorKernel, pt_abi.h pt_adaptive_update): one
// wave per 8x8 wave tile of the context's share (the whole image with world 1), which is the image's
// tile (y / 8) * tilesX + x / 8 of the two planes; a tile not yet retired takes err2 = the largest
// variance of the mean of its pixels' tone-mapped luminance and retires (retiredAt = frames) when
// frames >= minFrames and err2 <= thr2
struct TileErrorParams {
  Share share;
  int shardTiles;            // pt_frame.h shardTiles(share)
  int waveTiles;             // pt_frame.h waveTiles(share): the waves of the launch (0: a rank that owns nothing)
  int tilesX;                // image tiles per row, (width + 7) / 8
  const float4* accum;
  const float2* moments;
  float* err2;
  uint32_t* retiredAt;
  float kf;                  // (float)frames
  float limit;
  float thr2;                // threshold * threshold
  uint32_t frames;           // the frames the moments hold
  int minFrames;
};
hipError_t launchTileError(const TileErrorParams& p, hipStream_t s);

}  // namespace pt
