// pt_primary.hip -- camera-ray bins, and the camera-ray pass that reads them before a frame
// kernel (primaryKernel, liveListKernel; at the end). The bins: for one camera, the triangles each 8x8
// pixel tile's camera rays can hit, so the megakernel finds a camera ray's
// closest hit by testing its tile's few triangles (pass1.fsh hitTriangle
// IS:251-301, the same test as the traversal's) instead of walking the BVH
// (pt_kernels.hip primaryPacket).
//
// Every camera ray of pixel (px, py) leaves the eye through the image-plane
// point (x, y, -1.5) of camera space with x within a quarter pixel of the
// pixel's centre (IS:846-850: the AA jitter is +-0.5/W in NDC). A triangle
// point q (camera space, q = R^T (P - eye), R = cameraRotate's rotation) lies on
// such a ray iff it projects to that image point, and a hit needs t >= 0.0005
// (IS:281), so q.z < -2.5e-4 for every point a camera ray can hit. A triangle's
// bins are the tiles its projection -- clipped to q.z <= -2.5e-4 -- touches,
// widened by two pixels (far beyond the float rounding of the ray directions):
// conservative, so every triangle a camera ray hits is in its tile's bin.
// Results stay the reference's: a tie or an unreachable winner is retraced
// through the uploaded tree (as for the runtime tree, pt_trace.h refReachable).
//
// Build (once per camera and scene, on the frame's stream):
//   binRectKernel   per triangle: its tile rectangle (empty if off-screen / behind)
//   scan            per-triangle tile counts -> offsets (hipcub)
//   binCountKernel  per (triangle, tile) entry: count the tile's triangles
//   scan            per-tile counts -> bin starts (hipcub)
//   binFillKernel   per entry: place the triangle in its tile's bin
//   binGatherKernel per entry: its triangle's geometry record and leaf box, in bin order
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "pt_frame.h"
#include "pt_kernels.h"
#include "pt_trace.h"

namespace pt {

struct BinCam {
  double eye[3];
  double R[9];  // columns c0, c1, c2 of cameraRotate's upper 3x3
  int width, height, tilesX, tilesY;
};

constexpr double kNearZ = -2.5e-4;  // a hit point of a camera ray has q.z below this (t >= 0.0005)
constexpr double kMarginPx = 2.0;   // bins widened by this many pixels

__device__ __forceinline__ void toCam(const BinCam& c, const float4 v, double q[3]) {
  const double r0 = (double)v.x - c.eye[0], r1 = (double)v.y - c.eye[1], r2 = (double)v.z - c.eye[2];
  for (int a = 0; a < 3; a++) q[a] = c.R[3 * a] * r0 + c.R[3 * a + 1] * r1 + c.R[3 * a + 2] * r2;
}

// tile rectangle of triangle i -> rect[i] = (tx0, ty0, tx1, ty1) (tx0 > tx1: none), count[i] = its tiles
__global__ void binRectKernel(BinCam c, const float4* geo, int nTri, int4* rect, int* count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nTri) return;
  double q[3][3];
  for (int k = 0; k < 3; k++) toCam(c, geo[4 * (size_t)i + k], q[k]);
  // clip the triangle to q.z <= kNearZ (Sutherland-Hodgman, one plane): <= 4 points
  double px[4], py[4];
  int n = 0;
  for (int k = 0; k < 3; k++) {
    const double* a = q[k];
    const double* b = q[(k + 1) % 3];
    const bool ain = a[2] <= kNearZ, bin = b[2] <= kNearZ;
    if (ain) {
      px[n] = -1.5 * a[0] / a[2];
      py[n] = -1.5 * a[1] / a[2];
      n++;
    }
    if (ain != bin) {
      const double s = (kNearZ - a[2]) / (b[2] - a[2]);
      const double x = a[0] + s * (b[0] - a[0]), y = a[1] + s * (b[1] - a[1]);
      px[n] = -1.5 * x / kNearZ;
      py[n] = -1.5 * y / kNearZ;
      n++;
    }
  }
  int4 r = make_int4(1, 1, 0, 0);
  int cnt = 0;
  if (n > 0) {
    double x0 = 1e300, x1 = -1e300, y0 = 1e300, y1 = -1e300;
    for (int k = 0; k < n; k++) {
      // image plane -> pixel-centre coordinates (pix = (2 p + 1) / W - 1, IS:846)
      const double X = (px[k] + 1.0) * 0.5 * c.width - 0.5, Y = (py[k] + 1.0) * 0.5 * c.height - 0.5;
      x0 = fmin(x0, X); x1 = fmax(x1, X); y0 = fmin(y0, Y); y1 = fmax(y1, Y);
    }
    x0 -= kMarginPx; y0 -= kMarginPx; x1 += kMarginPx; y1 += kMarginPx;
    if (x1 >= 0.0 && y1 >= 0.0 && x0 <= c.width - 1.0 && y0 <= c.height - 1.0) {
      const int tx0 = (int)fmax(0.0, floor(x0 / 8.0)), ty0 = (int)fmax(0.0, floor(y0 / 8.0));
      const int tx1 = (int)fmin((double)(c.tilesX - 1), floor(x1 / 8.0));
      const int ty1 = (int)fmin((double)(c.tilesY - 1), floor(y1 / 8.0));
      if (tx0 <= tx1 && ty0 <= ty1) {
        r = make_int4(tx0, ty0, tx1, ty1);
        cnt = (tx1 - tx0 + 1) * (ty1 - ty0 + 1);
      }
    }
  }
  rect[i] = r;
  count[i] = cnt;
}

// entry e -> (triangle, tile): the triangle is the last one whose offset is <= e
__device__ __forceinline__ void entryOf(const int* offset, const int4* rect, int nTri, int tilesX, int e, int& tri,
                                        int& tile) {
  int lo = 0, hi = nTri - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (offset[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  tri = lo;
  const int4 r = rect[lo];
  const int k = e - offset[lo], w = r.z - r.x + 1;
  tile = (r.y + k / w) * tilesX + r.x + k % w;
}

__global__ void binCountKernel(const int* offset, const int4* rect, int nTri, int tilesX, int entries, int* tileCount) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  int tri, tile;
  entryOf(offset, rect, nTri, tilesX, e, tri, tile);
  atomicAdd(tileCount + tile, 1);
}

__global__ void binFillKernel(const int* offset, const int4* rect, int nTri, int tilesX, int entries, const int* binStart,
                              int* cursor, int* binTris) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  int tri, tile;
  entryOf(offset, rect, nTri, tilesX, e, tri, tile);
  binTris[binStart[tile] + atomicAdd(cursor + tile, 1)] = tri;
}

// per entry: its triangle's geometry record and reference leaf box, next to each other in bin order
__global__ void binGatherKernel(const int* binTris, int entries, const float4* geo, const float4* leafBox,
                                float4* binGeo, float4* binBox) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  const int i = binTris[e];
  for (int q = 0; q < 4; q++) binGeo[4 * (size_t)e + q] = geo[4 * (size_t)i + q];
  for (int q = 0; q < 2; q++) binBox[2 * (size_t)e + q] = leafBox[2 * (size_t)i + q];
}

// exclusive prefix sum of n ints in place-free form (out may not alias in); the total lands in out[n]
static hipError_t scanInts(const int* in, int* out, int n, void*& tmp, size_t& tmpBytes, hipStream_t s) {
  size_t need = 0;
  hipError_t e = hipcub::DeviceScan::ExclusiveSum(nullptr, need, in, out, n + 1, s);
  if (e != hipSuccess) return e;
  if (need > tmpBytes) {
    if (tmp) (void)hipFree(tmp);
    tmp = nullptr;
    e = hipMalloc(&tmp, need);
    if (e != hipSuccess) { tmpBytes = 0; return e; }
    tmpBytes = need;
  }
  return hipcub::DeviceScan::ExclusiveSum(tmp, need, in, out, n + 1, s);
}

hipError_t buildPrimaryBins(const float eye[3], const float cam[16], int width, int height, const float4* geo,
                            const float4* leafBox, int nTri, PrimaryBins& b, hipStream_t s) {
  // the camera-ray pass reads each bin entry's geometry and reference leaf box from the gathered
  // binGeo / binBox only (binGatherKernel): without leaf boxes it would test unwritten records
  if (!geo || !leafBox) return hipErrorInvalidValue;
  BinCam c;
  for (int a = 0; a < 3; a++) c.eye[a] = eye[a];
  // columns c0 = cam[0..2], c1 = cam[4..6], c2 = cam[8..10] (column-major, IS:849)
  for (int a = 0; a < 3; a++) {
    c.R[3 * a + 0] = cam[4 * a + 0];
    c.R[3 * a + 1] = cam[4 * a + 1];
    c.R[3 * a + 2] = cam[4 * a + 2];
  }
  c.width = width;
  c.height = height;
  c.tilesX = (width + 7) / 8;
  c.tilesY = (height + 7) / 8;
  const int nTiles = c.tilesX * c.tilesY;
  hipError_t e;
  auto grow = [&](auto*& p, size_t& cap, size_t need) -> hipError_t {
    if (need <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t r = hipMalloc(&p, need * sizeof(*p));
    if (r == hipSuccess) cap = need;
    return r;
  };
  if ((e = grow(b.rect, b.rectCap, (size_t)nTri)) != hipSuccess) return e;
  if ((e = grow(b.triCount, b.triCountCap, (size_t)nTri + 1)) != hipSuccess) return e;
  if ((e = grow(b.triOffset, b.triOffsetCap, (size_t)nTri + 1)) != hipSuccess) return e;
  if ((e = grow(b.tileCount, b.tileCountCap, (size_t)nTiles + 1)) != hipSuccess) return e;
  if ((e = grow(b.binStart, b.binStartCap, (size_t)nTiles + 1)) != hipSuccess) return e;
  const int B = 256;
  hipLaunchKernelGGL(binRectKernel, dim3((nTri + B - 1) / B), dim3(B), 0, s, c, geo, nTri, b.rect, b.triCount);
  if ((e = hipMemsetAsync(b.triCount + nTri, 0, sizeof(int), s)) != hipSuccess) return e;
  if ((e = scanInts(b.triCount, b.triOffset, nTri, b.tmp, b.tmpBytes, s)) != hipSuccess) return e;
  int entries = 0;  // the one host sync of a bin build (sizes the entry passes and the bin array)
  if ((e = hipMemcpyAsync(&entries, b.triOffset + nTri, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  if ((e = grow(b.binTris, b.binTrisCap, (size_t)std::max(entries, 1))) != hipSuccess) return e;
  if ((e = hipMemsetAsync(b.tileCount, 0, ((size_t)nTiles + 1) * sizeof(int), s)) != hipSuccess) return e;
  if (entries > 0)
    hipLaunchKernelGGL(binCountKernel, dim3((entries + B - 1) / B), dim3(B), 0, s, b.triOffset, b.rect, nTri, c.tilesX,
                       entries, b.tileCount);
  if ((e = scanInts(b.tileCount, b.binStart, nTiles, b.tmp, b.tmpBytes, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(b.tileCount, 0, ((size_t)nTiles + 1) * sizeof(int), s)) != hipSuccess) return e;  // cursors
  if (entries > 0)
    hipLaunchKernelGGL(binFillKernel, dim3((entries + B - 1) / B), dim3(B), 0, s, b.triOffset, b.rect, nTri, c.tilesX,
                       entries, b.binStart, b.tileCount, b.binTris);
  if ((e = grow(b.binGeo, b.binGeoCap, 4 * (size_t)std::max(entries, 1))) != hipSuccess) return e;
  if ((e = grow(b.binBox, b.binBoxCap, 2 * (size_t)std::max(entries, 1))) != hipSuccess) return e;
  if (entries > 0 && leafBox)
    hipLaunchKernelGGL(binGatherKernel, dim3((entries + B - 1) / B), dim3(B), 0, s, b.binTris, entries, geo, leafBox,
                       b.binGeo, b.binBox);
  b.tilesX = c.tilesX;
  b.tilesY = c.tilesY;
  b.entries = entries;
  return hipGetLastError();
}

// The pass tiles of a share (PrimaryBins::passList): wave tile w is one when its image tile has a
// non-empty bin -- a share tile wholly outside the image has none. One block walks the share's tiles
// in order, as liveListKernel walks a queue's items: a ballot per wave, the waves' counts summed
// through LDS, so the list is ascending. Its length lands behind it, at list[numItems].
constexpr int PASS_BS = 1024;
__global__ __launch_bounds__(PASS_BS) void passListKernel(Share share, int per, int numItems, const int* binStart,
                                                          int tilesX, int tilesY, int* list) {
  __shared__ int s_wave[PASS_BS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int base = 0;
  for (int w0 = 0; w0 < numItems; w0 += PASS_BS) {
    const int w = w0 + (int)threadIdx.x;
    bool in = false;
    if (w < numItems) {
      const int2 o = tileOrigin(share, w, per);
      const int tx = o.x >> 3, ty = o.y >> 3;
      if (tx < tilesX && ty < tilesY) in = binStart[ty * tilesX + tx + 1] > binStart[ty * tilesX + tx];
    }
    const unsigned long long b = __ballot(in);
    if (lane == 0) s_wave[wv] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < PASS_BS / 64; k++) {
      const int c = s_wave[k];
      before += k < wv ? c : 0;
      all += c;
    }
    if (in) list[base + before + __popcll(b & ((1ull << lane) - 1ull))] = w;
    base += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) list[numItems] = base;
}

hipError_t buildPassList(const Share& share, PrimaryBins& b, hipStream_t s) {
  const int numItems = waveTiles(share);
  b.passCount = 0;
  if (numItems <= 0) return hipSuccess;  // a rank that owns nothing
  if (!b.binStart) return hipErrorInvalidValue;
  hipError_t e;
  if ((size_t)numItems + 1 > b.passListCap) {
    if (b.passList) (void)hipFree(b.passList);
    b.passList = nullptr;
    b.passListCap = 0;
    if ((e = hipMalloc(&b.passList, ((size_t)numItems + 1) * sizeof(int))) != hipSuccess) return e;
    b.passListCap = (size_t)numItems + 1;
  }
  hipLaunchKernelGGL(passListKernel, dim3(1), dim3(PASS_BS), 0, s, share, shardTiles(share), numItems, b.binStart,
                     b.tilesX, b.tilesY, b.passList);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  int count = 0;  // the launches' grid: a second host sync of a bin build
  if ((e = hipMemcpyAsync(&count, b.passList + numItems, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  b.passCount = count;
  return hipSuccess;
}

void freePrimaryBins(PrimaryBins& b) {
  for (void* p : {(void*)b.rect, (void*)b.triCount, (void*)b.triOffset, (void*)b.tileCount, (void*)b.binStart,
                  (void*)b.binTris, (void*)b.binGeo, (void*)b.binBox, (void*)b.passList, b.tmp})
    if (p) (void)hipFree(p);
  b = PrimaryBins{};
}

// ------------------------------------------------------------ camera-ray pass
// Camera-ray pass: the bin path of primaryPacket (pt_kernels.hip) for every 8x8 tile of the
// rank, one wave per tile, before the megakernel. Inside the persistent
// megakernel (3 waves/SIMD) a tile's camera rays are a chain of dependent
// round trips (claim, bin, triangles, refReachable, env) that the few resident
// waves cannot hide; here a launch of one short wave per tile keeps up to 8
// waves per SIMD in flight and claims nothing. Sky pixels are finished here;
// every other pixel's result goes to primHit for the megakernel.
// In a pipelined launch a tile whose camera-ray bin is empty is not given to this pass: the
// running-mean update computes its samples (pt_kernels.h SkyTiles, pt_display.hip mixFrames). The
// grid is then passList's tiles x nFrames, and the other tiles' masks stay the zeros the runtime
// put there (pt_runtime.cpp bindBins). passList null: every tile of the share.
__global__ __launch_bounds__(64) void primaryKernel(RenderParams p, const int* passList) {
  __shared__ float4 s_tri[PT_PASS_BIN_CAP * 4];
  __shared__ float4 s_box[PT_PASS_BIN_CAP * 2];
  __shared__ int s_idx[PT_PASS_BIN_CAP];
  // block b: tile b / nFrames of frame b % nFrames (a batch's frames of one tile side by side).
  // (Blocks of 2 / 4 / 8 such one-wave items, fewer workgroups for the dispatcher: c2's 1/8 share of
  // a 20-frame batch 88.6 -> 92.2 / 93.4 / 102.2 us; one block per tile for several frames: DESIGN.md 3b.)
  const int fr = (int)(blockIdx.x % (unsigned)p.nFrames);
  const int item = (int)(blockIdx.x / (unsigned)p.nFrames);
  const int w = passList ? passList[item] : item;
  const int lane = threadIdx.x;
  if (p.zeroQueue && blockIdx.x == 0)  // the frame kernel's work-queue counters, zeroed for it (it runs next on this stream)
    for (int q = lane; q < NUM_QUEUES; q += 64) p.queue[q * CTL_LINE_INTS] = 0;
  const int2 o = tileOrigin(shareOf(p), w, p.shardTiles);
  const int px = o.x + (lane & 7);
  const int py = o.y + (lane >> 3);
  const bool valid = px < p.width && py < p.height;
  const int tx = o.x >> 3, ty = o.y >> 3;
  int b0 = 0, b1 = 0;  // a tile wholly outside the image has no bin (and no valid lane)
  // PT_FLAG_ADAPTIVE: the frame count at which the tile retired (pt_adaptive.hip; the bins' tiles are the
  // image's: ty * tilesX + tx), read beside the bin's bounds -- three scalar loads in one round trip
  uint32_t gone = 0u;
  if (tx < p.binTilesX && ty < p.binTilesY) {
    b0 = p.binStart[ty * p.binTilesX + tx];
    b1 = p.binStart[ty * p.binTilesX + tx + 1];
    if (p.retiredAt) gone = p.retiredAt[ty * p.binTilesX + tx];
  }
  // a retired tile takes no sample: an empty mask, so no frame kernel claims it, no sky colour stored,
  // no ray counted
  if (gone != 0u) {
    if (lane == 0) p.primMask[(size_t)fr * p.numItems + w] = 0ull;
    return;
  }
  const int n = b1 - b0;
  // the tile's results compacted (RenderParams::primMask): the slots that need a path, in slot order
  int2* out = p.primHit + ((size_t)fr * p.numItems + w) * 64;
  unsigned long long* mask = p.primMask + (size_t)fr * p.numItems + w;
  const FrameRef fp = frameRef(p, fr);  // this block's frame (storeSample's colour buffer)
  if (n > PT_PASS_BIN_CAP) {  // the frame kernel traces this tile's camera rays (the megakernel as a packet)
    const unsigned long long m = __ballot(valid);
    if (valid) out[__popcll(m & ((1ull << lane) - 1ull))] = make_int2(PRIM_TILE, 0);
    if (lane == 0) *mask = m;
    return;
  }
  // the bin's triangles and their leaf boxes in bin order (binGeo / binBox, gathered at bin build): one
  // round trip after binStart instead of binTris -> geo, and refReachable's leaf box from LDS
  // (an empty bin -- every camera ray of the tile is sky -- stages nothing and needs no barrier)
  if (n > 0) {
    for (int t = lane >> 2; t < n; t += 16) {  // one float4 of one triangle (and of its leaf box) per lane
      s_tri[4 * t + (lane & 3)] = p.binGeo[4 * (size_t)(b0 + t) + (lane & 3)];
      if ((lane & 3) < 2) s_box[2 * t + (lane & 3)] = p.binBox[2 * (size_t)(b0 + t) + (lane & 3)];
      else if ((lane & 3) == 2) s_idx[t] = p.binTris[b0 + t];
    }
    __syncthreads();
  }
  uint32_t seed;
  const V3 dir = cameraRay(p, fp.sampleIndex, valid ? px : 0, valid ? py : 0, seed);
  const V3 eye = v3(p.eye[0], p.eye[1], p.eye[2]);
  float tbest;
  int best;
  bool tie;
  closestInBin(n, valid, eye, dir, [&](int k) { return s_tri + 4 * k; }, tbest, best, tie);
  uint32_t rays = 0;
  int res = PRIM_MISS;
  if (valid) {
    res = best >= 0 ? s_idx[best] : PRIM_MISS;
    if (tie || (res >= 0 && !refReachableBox(p.scene, s_box[2 * best], s_box[2 * best + 1], eye, dir, tbest))) {
      res = PRIM_RETRACE;  // counted by the megakernel's retrace
    } else {
      rays = 1;
      if (res == PRIM_MISS) storeSample(p, fp, px, py, sampleHdr(p.env, dir));
    }
  }
  const bool need = valid && res != PRIM_MISS;
  const unsigned long long m = __ballot(need);
  if (need) out[__popcll(m & ((1ull << lane) - 1ull))] = make_int2(res, __float_as_int(tbest));
  if (lane == 0) *mask = m;
  addRays(p.rayShards, rays);
}

hipError_t launchPrimary(const RenderParams& p, const int* passList, int passCount, hipStream_t s) {
  if (!p.primHit || !p.primMask || !p.binStart || !p.binGeo || !p.binBox || p.numItems <= 0) return hipErrorInvalidValue;
  if (passList && (passCount <= 0 || passCount > p.numItems)) return hipErrorInvalidValue;
  const unsigned tiles = passList ? (unsigned)passCount : (unsigned)p.numItems;
  hipLaunchKernelGGL(primaryKernel, dim3(tiles * (unsigned)p.nFrames), dim3(64), 0, s, p, passList);
  return hipGetLastError();
}

// Live-item lists (RenderParams::liveItems): block q walks work queue q's items in claim order
// (TileCursor::next: item `it` is tile q * perQueue + it / nFrames of frame it % nFrames) and keeps,
// in that order, those whose camera-ray mask is not 0 -- a ballot per wave, the waves' counts
// summed through LDS -- so a regen wave's claim never lands on a tile the pass has finished
// (c2 at 1080p: 55 % of the tiles are all sky, c3 96 %). The list is a function
// of the masks alone: the same items in the same order on every run.
constexpr int LIVE_BS = 1024;
__global__ __launch_bounds__(LIVE_BS) void liveListKernel(RenderParams p) {
  __shared__ int s_wave[LIVE_BS / 64];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nF = p.nFrames, total = p.perQueue * nF;
  uint4* seg = p.liveItems + (size_t)q * liveStride(p.perQueue, nF);
  uint4* out = seg + LIVE_HEAD;
  auto load = [&](int it, int& t, int& fr) -> unsigned long long {
    const int k = it / nF;
    fr = it - k * nF;
    t = q * p.perQueue + k;
    return it < total && t < p.numItems ? p.primMask[(size_t)fr * p.numItems + t] : 0ull;
  };
  int base = 0;  // live items of the rounds before this one
  int t, fr;
  unsigned long long m = load((int)threadIdx.x, t, fr);
  for (int it0 = 0; it0 < total; it0 += LIVE_BS) {
    int tn, frn;  // the next round's mask, in flight across this round's barriers
    const unsigned long long mn = load(it0 + LIVE_BS + (int)threadIdx.x, tn, frn);
    const unsigned long long b = __ballot(m != 0);
    if (lane == 0) s_wave[wv] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < LIVE_BS / 64; w++) {
      const int c = s_wave[w];
      before += w < wv ? c : 0;
      all += c;
    }
    if (m != 0)
      out[base + before + __popcll(b & ((1ull << lane) - 1ull))] = make_uint4((uint32_t)t, (uint32_t)fr, (uint32_t)m, (uint32_t)(m >> 32));
    base += all;
    __syncthreads();
    m = mn;
    t = tn;
    fr = frn;
  }
  if (threadIdx.x == 0) seg[0] = make_uint4((uint32_t)base, 0u, 0u, 0u);  // the count, on the segment's first line
}

hipError_t launchLiveList(const RenderParams& p, hipStream_t s) {
  if (!p.primMask || !p.liveItems || p.numItems <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(liveListKernel, dim3(NUM_QUEUES), dim3(LIVE_BS), 0, s, p);
  return hipGetLastError();
}

}  // namespace pt
