// pt_kernels.hip -- the megakernel of the progressive path tracer on MI355X (gfx950): a tile's
// camera rays and paths, and the tile reorder between frames. The three pass1.fsh integrators are
// pt_paths.h (the radiance query runs them too). What it shares with the other frame kernels (the pixel's
// seed, camera ray and store, the share's tiles) is pt_frame.h; traversal is pt_trace.h.
// Each launcher follows its kernel.
//
// Execution model (DESIGN.md "Kernels"):
//  * persistent grid sized to residency; each wave64 dequeues 8x8 pixel tiles
//    from 8 per-XCD-group work counters (blockIdx % 8), stealing when its own
//    queue drains;
//  * one lane per pixel runs the whole path (megakernel): ray gen, closest-hit
//    traversal, env any-hit shadow rays, BRDF/MIS, running-mean accumulate;
//  * traversal keeps the current node in registers and the deferred siblings in
//    an LDS stack (LDS_STACK entries per lane, lane-interleaved so a wave's
//    push/pop is bank-conflict free) that spills to a per-thread HBM region
//    only for trees deeper than LDS_STACK;
//  * node records are re-laid out at upload as 64-byte "wide" records holding
//    both children's boxes (one dependent fetch per visited internal node
//    instead of the reference's three); triangles as 64-byte records with the
//    precomputed unit normal and plane offset.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_paths.h"
#include "pt_scene.h"
#include "pt_trace.h"

namespace pt {

// main IS:844-872 for one pixel (px, py from the bottom-left), in two parts:
// the camera ray (pt_frame.h cameraRay + primaryPixel) and the rest of the path
// (finishPixel, which recomputes the camera ray and RNG state from the pixel).
// f: the frame the pixel belongs to (its sample index and colour buffer); a counting
// launch mixes into the running mean in place and counts the read
__device__ __forceinline__ void accumulate(const RenderParams& p, const FrameRef& f, int px, int py, V3 color, Counters& C,
                                           bool count) {
  FrameRef g = f;
  if (count) {
    g.col = nullptr;
    C.texels++;
  }
  storeSample(p, g, px, py, color);
}

// the camera ray's closest hit; a miss is finished here (sky colour accumulated)
template <bool CULL, bool COUNT>
__device__ __forceinline__ int primaryPixel(const RenderParams& p, const FrameRef& f, int px, int py, Stack& st,
                                            Counters& C, const float4* top, float& t) {
  uint32_t seed;
  const V3 dir = cameraRay(p, f.sampleIndex, px, py, seed);
  const V3 eye = v3(p.eye[0], p.eye[1], p.eye[2]);
  Tracer<CULL, COUNT> tr{p.scene, st, C, top};
  const int tri = tr.trace(eye, dir, t);
  if (tri < 0) {
    const V3 color = sampleHdr(p.env, dir);
    if (COUNT) C.texels++;
    accumulate(p, f, px, py, color, C, COUNT);
  }
  return tri;
}

// primaryPixel for a whole wave: the camera rays of the wave's pixels traced as
// one packet (tracePacket); a ray that met an exact tie is retraced in the
// reference order. All 64 lanes call it; valid marks the lanes with a pixel.
template <bool CULL>
__device__ __forceinline__ int primaryPacket(const RenderParams& p, const FrameRef& f, int px, int py, bool valid,
                                             Stack& st, Counters& C, const float4* top, PacketEntry* pstack, float& t) {
  uint32_t seed;
  const V3 dir = cameraRay(p, f.sampleIndex, valid ? px : 0, valid ? py : 0, seed);
  const V3 eye = v3(p.eye[0], p.eye[1], p.eye[2]);
  bool tie;
  int tri;
  // camera-ray bins (pt_primary.hip): the tile's candidate triangles, each tested
  // with hitTriangle's exact arithmetic (IS:251-301); the closest stands when no
  // other candidate ties it and the reference traversal reaches it (refReachable),
  // else the ray is retraced in the reference order
  int b0 = 0, b1 = 0;  // an 8x8 tile of a shard wholly outside the image (no valid lane) has no bin
  if (p.binStart) {
    // every lane calls this function, so the first active lane is lane 0, whose pixel lies in the tile
    const int tx = __builtin_amdgcn_readfirstlane(px) >> 3, ty = __builtin_amdgcn_readfirstlane(py) >> 3;
    if (tx < p.binTilesX && ty < p.binTilesY) {
      const int tile = ty * p.binTilesX + tx;
      b0 = p.binStart[tile];
      b1 = p.binStart[tile + 1];
    }
  }
  if (p.binStart && b1 - b0 <= PT_BIN_CAP) {
    // the bin's triangles staged in the wave's own (still empty) part of the LDS stack:
    // every lane loads one float4 of one triangle, so the whole bin costs two memory round
    // trips instead of one per triangle; the test loop then reads broadcast LDS records.
    // Triangle t's 16 floats at wb + (t >> 2) * BLOCK + (t & 3) * 16, its index at row IDX.
    constexpr int IDX = (PT_BIN_CAP + 3) / 4;
    static_assert(PT_BIN_CAP <= 64 && IDX < LDS_STACK, "bin staging fits the wave's stack rows 0..IDX");
    const int n = b1 - b0;
    int* wb = st.lds - __lane_id();  // column 0 of this wave's stack columns
    const int lane = __lane_id();
    for (int t = lane >> 2; t < n; t += 16) {
      const int i = p.binTris[b0 + t];
      const float4 v = p.scene.geo[4 * (size_t)i + (lane & 3)];
      *reinterpret_cast<float4*>(wb + (t >> 2) * BLOCK + (t & 3) * 16 + 4 * (lane & 3)) = v;
      if ((lane & 3) == 0) wb[IDX * BLOCK + t] = i;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float tbest;
    int best;
    closestInBin(n, valid, eye, dir,
                 [&](int k) { return reinterpret_cast<const float4*>(wb + (k >> 2) * BLOCK + (k & 3) * 16); }, tbest, best,
                 tie);
    if (best >= 0) best = wb[IDX * BLOCK + best];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // every lane has read the staging before the stack is used
    __builtin_amdgcn_wave_barrier();
    if (valid) C.rays++;
    tri = best;
    t = tbest;
    if (valid && (tie || (tri >= 0 && !refReachable(p.scene, tri, eye, dir, t)))) {
      C.rays--;  // the same ray, counted once
      tri = traceRay<false, CULL, false, Stack>(p.scene, eye, dir, t, st, C);
    }
  } else if (!p.packets) {  // a tree too deep for the packet stack: each ray on its own
    tri = -1;
    if (valid) {
      Tracer<CULL, false> tr{p.scene, st, C, top};
      tri = tr.trace(eye, dir, t);
    }
  } else if (p.scene.fast) {  // through the runtime's tree, checked against the reference's
    // (the block's LDS holds the 4-wide tree's top, not this binary tree's: no top)
    const int pos = tracePacket<CULL, NODE_FUSED>(fastView(p.scene), eye, dir, valid, t, tie, pstack, C, nullptr);
    tri = pos >= 0 ? p.scene.fastTri[pos] : -1;
    if (valid && (tie || (tri >= 0 && !refReachable(p.scene, tri, eye, dir, t)))) {
      C.rays--;  // the same ray, counted once
      tri = traceRay<false, CULL, false, Stack>(p.scene, eye, dir, t, st, C);
    }
  } else {
    tri = tracePacket<CULL>(p.scene, eye, dir, valid, t, tie, pstack, C, top);
    if (valid && tie) {
      C.rays--;
      tri = traceRay<false, CULL, false, Stack, true>(p.scene, eye, dir, t, st, C, false, top);
    }
  }
  if (valid && tri < 0) {
    const V3 color = sampleHdr(p.env, dir);
    accumulate(p, f, px, py, color, C, false);
  }
  return tri;
}

// the rest of the path of a pixel whose camera ray hit triangle tri at t
template <int INTEG, bool CULL, bool COUNT>
__device__ __forceinline__ void finishPixel(const RenderParams& p, const FrameRef& f, int px, int py, int tri, float t,
                                            Stack& st, Counters& C, const float4* top) {
  Tracer<CULL, COUNT> tr{p.scene, st, C, top};
  uint32_t seed;
  const uint32_t sampleIndex = f.sampleIndex;
  const V3 dir = cameraRay(p, sampleIndex, px, py, seed);  // the same ray and RNG state as primaryPixel
  const V3 eye = v3(p.eye[0], p.eye[1], p.eye[2]);
  Hit first;
  finishHit(p.scene, tri, eye, dir, t, first);
  V3 Li;
  if (INTEG == 0) Li = pathLambert(tr, p.env, first, p.maxBounce, seed, C, COUNT);
  else if (INTEG == 1) Li = pathDisneyUniform(tr, p.env, first, p.maxBounce, seed, C, COUNT);
  else Li = pathMIS(tr, p.env, first, p.maxBounce, seed, px, py, sampleIndex, C, COUNT);
  // MIS (8-16 bounces): the camera hit's emission reloaded once the path has ended rather than
  // held across every bounce (the megakernel at its 168-VGPR limit: 37 -> 28 VGPRs spilled)
  const V3 Le0 = INTEG == 2 ? emissiveOf(p.scene, tri) : first.m.emissive;
  accumulate(p, f, px, py, Le0 + Li, C, COUNT);
}

// ------------------------------------------------------------ tile order
// One block per queue band, between frames: build the next frame's work items
// (TileCursor) from the costs the megakernel measured in this one.
//  * Split state: a wave runs its item's paths in lock step, so a tile whose
//    lanes take turns at long traversals lasts the sum of its slowest lanes --
//    for a few tiles most of a frame. A tile whose longest item cost more than
//    splitPct % of a wave's share of the band (band cost / waves per band)
//    is split once more (2^lg items of 64 >> lg pixels, lg <= 6); one whose
//    items became cheap (< 1/4 of that) is merged back one step.
//  * Order: items by their tile's longest item, descending, so the long ones
//    start first: a counting sort over 128 cost buckets (the cost's octave and
//    two more bits, ~19 % wide; order within a bucket is arbitrary) -- one pass
//    of LDS atomics instead of a bitonic sort's 55 barrier phases. Progressive
//    frames share camera and scene, so this frame's costs predict the next's.
// group > 1 sorts groups of consecutive tiles by summed cost and never splits.
constexpr int REORDER_BUCKETS = 128;
__device__ __forceinline__ int costBucket(unsigned long long c) {  // 0 = most expensive
  const unsigned v = (unsigned)min(c, 0xffffffffull) | 1u;
  const int oct = 31 - __clz(v);
  const int frac = oct >= 2 ? (int)((v >> (oct - 2)) & 3u) : (int)((v << (2 - oct)) & 3u);
  return REORDER_BUCKETS - 1 - (oct * 4 + frac);
}
__global__ __launch_bounds__(1024) void reorderKernel(int* cost, int* costMax, int* splitLg, int* ema, int* order,
                                                       int perQueue,
                                                       int orderCap, int numItems, int group, int numWaves,
                                                       int splitPct) {
  __shared__ int bucketOf[REORDER_MAX];  // each group's bucket
  __shared__ int rankG[REORDER_MAX];     // the group at each rank, most expensive first
  __shared__ int start[REORDER_BUCKETS];
  __shared__ int scan[1024];
  __shared__ int partialPos;
  __shared__ unsigned long long sumCost;
  const int q = blockIdx.x;
  const int base = q * perQueue;
  const int n = max(0, min(perQueue, numItems - base));
  const int ng = (n + group - 1) / group;  // groups of `group` consecutive tiles (the last may be short)
  const int lastSize = n - (ng - 1) * group;
  const bool splitting = group == 1 && splitLg != nullptr && splitPct > 0;
  if (threadIdx.x == 0) sumCost = 0;
  if (threadIdx.x < REORDER_BUCKETS) start[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long mySum = 0;
  for (int g = threadIdx.x; g < ng; g += blockDim.x) {
    const int t0 = base + g * group, t1 = min(t0 + group, base + n);
    for (int t = t0; t < t1; t++) mySum += (unsigned)max(cost[t], 0);
  }
  atomicAdd(&sumCost, mySum);
  __syncthreads();
  // a wave's share of the band's work: the cost above which an item forms the tail
  const unsigned long long share = sumCost / (unsigned long long)max(1, numWaves / NUM_QUEUES);
  const unsigned long long target = max(share * (unsigned long long)splitPct / 100ull, 1ull);
  for (int g = threadIdx.x; g < ng; g += blockDim.x) {
    unsigned long long c = 0;
    const int t0 = base + g * group, t1 = min(t0 + group, base + n);
    if (splitting) {
      const int t = t0;
      const unsigned long long m = (unsigned)max(costMax[t], 1);
      int lg = splitLg[t];
      if (m > target && lg < MAX_SPLIT_LG) lg++;
      else if (lg > 0 && 4 * m < target) lg--;
      splitLg[t] = lg;
      c = m;
      costMax[t] = 0;
    } else {
      for (int t = t0; t < t1; t++) c += (unsigned)max(cost[t], 1);
      if (costMax)
        for (int t = t0; t < t1; t++) costMax[t] = 0;
    }
    for (int t = t0; t < t1; t++) cost[t] = 0;
    if constexpr (PT_COST_EMA > 0) {  // a path's cost varies frame to frame: rank by the running estimate
      const unsigned long long e = (unsigned)ema[base + g];
      constexpr int S = PT_COST_EMA > 0 ? PT_COST_EMA : 1;  // weight of this frame: 2^-S
      c = e ? (((1ull << S) - 1) * e + min(c, 0x7fffffffull) + (1ull << (S - 1))) >> S : min(c, 0x7fffffffull);
      ema[base + g] = (int)c;
    }
    const int bk = costBucket(c);
    bucketOf[g] = bk;
    atomicAdd(&start[bk], 1);
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // exclusive scan of the bucket counts, one wave
    const int lane = threadIdx.x;
    const int c0 = start[2 * lane], c1 = start[2 * lane + 1];
    int incl = c0 + c1;
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off, 64);
      if (lane >= off) incl += v;
    }
    const int excl = incl - c0 - c1;
    start[2 * lane] = excl;
    start[2 * lane + 1] = excl + c0;
  }
  __syncthreads();
  for (int g = threadIdx.x; g < ng; g += blockDim.x) rankG[atomicAdd(&start[bucketOf[g]], 1)] = g;
  __syncthreads();
  int* out = order + (size_t)q * orderCap;
  if (splitting) {
    // item offsets: exclusive scan of 2^lg over the ranks (ceil(ng / 1024) ranks per thread)
    const int per = (ng + 1023) / 1024;
    const int r0 = min(ng, (int)threadIdx.x * per), r1 = min(ng, r0 + per);
    int local = 0;
    for (int r = r0; r < r1; r++) local += 1 << splitLg[base + rankG[r]];
    scan[threadIdx.x] = local;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const int v = threadIdx.x >= (unsigned)off ? scan[threadIdx.x - off] : 0;
      __syncthreads();
      scan[threadIdx.x] += v;
      __syncthreads();
    }
    const int total = scan[1023];
    if (total <= orderCap) {
      int pos = scan[threadIdx.x] - local;
      for (int r = r0; r < r1; r++) {
        const int t = base + rankG[r];
        const int lg = splitLg[t];
        for (int sIdx = 0; sIdx < (1 << lg); sIdx++) out[pos++] = t | sIdx << ITEM_TILE_BITS | lg << 28;
      }
      if (threadIdx.x == 0) order[(size_t)NUM_QUEUES * orderCap + q] = total;
      return;
    }
    // no room: this frame unsplit, and the band starts over
    for (int r = threadIdx.x; r < ng; r += blockDim.x) splitLg[base + r] = 0;
  }
  for (int r = threadIdx.x; r < ng; r += blockDim.x)
    if (rankG[r] == ng - 1) partialPos = r;
  __syncthreads();
  for (int r = threadIdx.x; r < ng; r += blockDim.x) {
    const int g = rankG[r];
    const int off = r * group - (r > partialPos ? group - lastSize : 0);
    const int len = g == ng - 1 ? lastSize : group;
    for (int k = 0; k < len; k++) out[off + k] = base + g * group + k;
  }
  if (threadIdx.x == 0) order[(size_t)NUM_QUEUES * orderCap + q] = n;
}

hipError_t launchReorder(int* cost, int* costMax, int* splitLg, int* ema, int* order, int perQueue, int orderCap,
                         int numItems, int group, int numWaves, int splitPct, hipStream_t s) {
  if ((perQueue + group - 1) / group > REORDER_MAX || orderCap < perQueue) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reorderKernel, dim3(NUM_QUEUES), dim3(1024), 0, s, cost, costMax, splitLg, ema, order, perQueue,
                     orderCap, numItems, group, numWaves, splitPct);
  return hipGetLastError();
}

// ------------------------------------------------------------ render kernel
__device__ __forceinline__ uint32_t waveSum(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// WAVES > 0: compiled for that many waves per SIMD (the latency-bound large
// scenes' variant, pt_runtime.cpp renderOne)
template <int INTEG, bool CULL, bool COUNT, int WAVES = 0>
__global__ __launch_bounds__(BLOCK, WAVES > 0 ? WAVES
                                             : (INTEG == 0 ? PT_MIN_WAVES_LAMBERT
                                                           : INTEG == 2 ? PT_MIN_WAVES_MIS : PT_MIN_WAVES)) void renderKernel(
    RenderParams p) {
  __shared__ int s_stack[LDS_STACK * BLOCK];
  Stack st;
  st.init(s_stack, p.ovf, p.ovfDepth);
  st.reset();
  __shared__ unsigned s_drained;  // the work queues this block's waves found drained (TileCursor)
  if (threadIdx.x == 0) s_drained = 0;
  // the top of the tree (every ray's first node visits) staged in LDS once per block
  __shared__ float4 s_nodes[LDS_NODES * 4];
  {
    const bool w4 = !COUNT && p.scene.fast;  // the 4-wide tree's top
    // the tree the per-ray walks traverse first. (A fetch-counting launch never has p.scene.fast set,
    // renderOne: the fbvh / fnTop arm, the binary runtime tree's, is never taken. Without it the COUNT
    // kernels' code is 52 bytes shorter; it stays until a change means to alter them, DESIGN.md.)
    const float4* src = w4 ? p.scene.fbvh4 : p.scene.fast ? p.scene.fbvh : p.scene.bvh;
    // the copy's size from the staged tree's own record kind (never the other tree's: DESIGN.md §8)
    const int n = w4 ? p.scene.f4nTop * W4_F4 : p.scene.fast ? p.scene.fnTop * 4 : p.scene.nTop * 4;
    for (int i = threadIdx.x; i < n; i += BLOCK) s_nodes[i] = src[i];
  }
  __syncthreads();
  const float4* top = s_nodes;
  Counters C = {0, 0, 0, 0, 0};
  const int lane = threadIdx.x & 63;
  const int home = blockIdx.x & (NUM_QUEUES - 1);
  __shared__ PacketEntry s_packet[BLOCK / 64][COUNT ? 1 : PKT_DEPTH];  // camera-ray packet stacks
  PacketEntry* pstack = s_packet[threadIdx.x >> 6];
#if PT_WAVE_TRACE
  const unsigned long long wStart = wall_clock64();
  unsigned long long wTiles = 0, wLongest = 0, wLongestAt = 0, wNodeIt = 0, wLeafIt = 0;
#endif
  TileCursor cur;
  cur.drained = &s_drained;
  // Each lane runs its pixel's whole path right after the tile's camera rays.
  // (Deferring the paths of the pixels that hit something to a per-wave LDS
  // queue and running them 64 at a time keeps every lane busy, but it mixes
  // tiles: 64-path batches made c2 0.77 ms instead of 0.55, 32-path batches
  // 0.59 -- the coherence of one tile's rays is worth more than full lanes.)
  int fr = 0;  // the claimed item's frame in the launch's batch
  int item = cur.next(p.queue, p.perQueue, p.numItems, home, fr, p.nFrames, p.tileOrder, p.orderCap);
  while (item >= 0) {
    const FrameRef fv = frameRef(p, fr);  // the item's frame: its sample index and colour buffer (accumulate)
    const int w = itemTile(item);
    const long long t0 = COUNT ? 0 : clock64();
#if PT_WAVE_TRACE
    const unsigned long long tw0 = wall_clock64();
    const uint32_t n0 = C.nodes, l0 = C.tris, m0 = C.mats;
#endif
    const int2 o = tileOrigin(shareOf(p), w, p.shardTiles);
    // a split item runs pixels [sub * n, (sub + 1) * n) of the tile (n = 64 >> lg), one per lane
    const int lg = itemLg(item), nLanes = 64 >> lg;
    const int k = itemSub(item) * nLanes + lane;
    const int px = o.x + (k & 7);
    const int py = o.y + (k >> 3);
    const bool valid = lane < nLanes && px < p.width && py < p.height;
    if (!COUNT && p.primHit) {  // camera rays already traced by primaryKernel
      const unsigned long long pm = primTileMask(p, fr, w);
      const int2 h = valid ? primOfSlot(pm, primTileEntries(p, fr, w), k) : make_int2(PRIM_MISS, 0);
      int tri = h.x;
      float t = __int_as_float(h.y);
      if (__ballot(valid && tri == PRIM_TILE)) {  // wave-uniform: the whole tile
        tri = primaryPacket<CULL>(p, fv, px, py, valid, st, C, top, pstack, t);
      } else if (valid && tri == PRIM_RETRACE) {  // in the reference order, as primaryPacket does
        uint32_t seed;
        const V3 dir = cameraRay(p, fv.sampleIndex, px, py, seed);
        const V3 eye = v3(p.eye[0], p.eye[1], p.eye[2]);
        tri = traceRay<false, CULL, false, Stack>(p.scene, eye, dir, t, st, C);
        if (tri < 0) accumulate(p, fv, px, py, sampleHdr(p.env, dir), C, false);
      }
      if (valid && tri >= 0) finishPixel<INTEG, CULL, COUNT>(p, fv, px, py, tri, t, st, C, top);
    } else if (!COUNT && (p.packets || p.binStart)) {
      float t;
      const int tri = primaryPacket<CULL>(p, fv, px, py, valid, st, C, top, pstack, t);
      if (valid && tri >= 0) finishPixel<INTEG, CULL, COUNT>(p, fv, px, py, tri, t, st, C, top);
    } else if (valid) {
      float t;
      const int tri = primaryPixel<CULL, COUNT>(p, fv, px, py, st, C, top, t);
      if (tri >= 0) finishPixel<INTEG, CULL, COUNT>(p, fv, px, py, tri, t, st, C, top);
    }
    if (!COUNT && p.tileCost && lane == 0) {
      const int dt = (int)min(clock64() - t0, (long long)0x3fffffff);
      atomicAdd(p.tileCost + w, dt);
      atomicMax(p.tileCostMax + w, dt);
    }
#if PT_WAVE_TRACE
    const unsigned long long tEnd = wall_clock64();
    wTiles++;
    uint32_t dn = C.nodes - n0, dl = C.tris - l0, dw = C.mats - m0;
    for (int off = 32; off > 0; off >>= 1) dw += (uint32_t)__shfl_xor(dw, off, 64);
    for (int off = 32; off > 0; off >>= 1) {
      dn = max(dn, (uint32_t)__shfl_xor(dn, off, 64));
      dl = max(dl, (uint32_t)__shfl_xor(dl, off, 64));
    }
    if (tEnd - tw0 > wLongest) {
      wNodeIt = dn;
      wLeafIt = dl | (unsigned long long)dw << 32;
      wLongest = tEnd - tw0;
      wLongestAt = (unsigned long long)__shfl(px, 0, 64) << 16 | (unsigned long long)__shfl(py, 0, 64);
    }
#endif
    item = cur.next(p.queue, p.perQueue, p.numItems, home, fr, p.nFrames, p.tileOrder, p.orderCap);
  }
#if PT_WAVE_TRACE
  if (p.waveTrace && lane == 0) {
    unsigned long long* r = p.waveTrace + 6 * ((size_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6));
    r[0] = wStart; r[1] = wall_clock64(); r[2] = wTiles | wLongestAt << 32; r[3] = wLongest;
    r[4] = wNodeIt; r[5] = wLeafIt;
  }
#endif
  addRays(p.rayShards, C.rays);
  if (COUNT) {
    uint32_t n = waveSum(C.nodes), t = waveSum(C.tris), m = waveSum(C.mats), x = waveSum(C.texels);
    if (lane == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + 1), (unsigned long long)n);
      atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + 2), (unsigned long long)t);
      atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + 3), (unsigned long long)m);
      atomicAdd(reinterpret_cast<unsigned long long*>(p.stats + 4), (unsigned long long)x);
    }
  }
}

// ------------------------------------------------------------ launchers
// The megakernel instantiation of a frame, for the occupancy query that sizes the grid and for the
// launch alike: counting launches never cull; the wide (WIDE_WAVES) variant is the culling Disney / MIS one
template <int I>
static const void* renderVariantI(bool cull, bool count, bool wide) {
  if (count) return (const void*)renderKernel<I, false, true>;
  if (cull && wide && I != 0) return (const void*)renderKernel<I, true, false, WIDE_WAVES>;
  return cull ? (const void*)renderKernel<I, true, false> : (const void*)renderKernel<I, false, false>;
}
static const void* renderVariant(int integrator, bool cull, bool count, bool wide) {
  return integrator == 0   ? renderVariantI<0>(cull, count, wide)
         : integrator == 1 ? renderVariantI<1>(cull, count, wide)
                           : renderVariantI<2>(cull, count, wide);
}

hipError_t launchRender(const RenderParams& p, int integrator, int grid, hipStream_t s, bool cull, bool count,
                        bool wide) {
  void* args[] = {const_cast<RenderParams*>(&p)};
  (void)hipLaunchKernel(renderVariant(integrator, cull, count, wide), dim3(grid), dim3(BLOCK), args, 0, s);
  return hipGetLastError();
}

hipError_t renderBlocksPerCU(int integrator, bool cull, bool count, bool wide, int* nb) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, renderVariant(integrator, cull, count, wide), BLOCK, 0);
}

}  // namespace pt
