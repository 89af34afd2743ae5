// pt_frame.h -- what every frame kernel knows about a pixel, each stated once: which pixels a
// context's screen-tile share (pt_kernels.h Share) holds and in what order, the pixel's seed and
// camera ray, its frame of a batch and the store of its sample, and the closest triangle of a bin. The megakernel (pt_kernels.hip), the regen kernel
// (pt_regen.hip), the camera-ray pass (pt_primary.hip), the guide pass (pt_guides.hip) and the
// pack / mix kernels (pt_display.hip) call these, so their agreeing bit for bit per pixel rests on
// one text. The Share functions are host code too (pt_runtime.cpp, tests/native/share_table.cpp).
#pragma once
#include "pt_kernels.h"

namespace pt {

// ------------------------------------------------------------ the share
// The one place a Share is filled (tileSize a multiple of 8; rank < world).
__host__ __device__ inline Share makeShare(int width, int height, int tileSize, int rank, int world) {
  return Share{width, height, tileSize, (width + tileSize - 1) / tileSize, rank, world};
}
__host__ __device__ inline int shardsY(const Share& s) { return (s.height + s.shardSize - 1) / s.shardSize; }
// shard tiles g = j * world + rank, j = 0 .. ownedShards - 1 (0: a rank past the last shard owns nothing)
__host__ __device__ inline int ownedShards(const Share& s) {
  return (s.shardsX * shardsY(s) - s.rank + s.world - 1) / s.world;
}
// pixels of the owned shard tiles, those outside the image included: slot k is pixel
// (k % shardSize^2) of the share's (k / shardSize^2)-th shard tile, rows first
__host__ __device__ inline long slots(const Share& s) { return (long)ownedShards(s) * s.shardSize * s.shardSize; }
__host__ __device__ inline int shardTiles(const Share& s) { return (s.shardSize >> 3) * (s.shardSize >> 3); }
// 8x8 wave tiles of the share: slots / 64 (RenderParams::numItems)
__host__ __device__ inline int waveTiles(const Share& s) { return ownedShards(s) * shardTiles(s); }

// A frame's parameter block carries its Share as six fields; these are the only two places that know which
__host__ __device__ inline Share shareOf(const RenderParams& p) {
  Share s;
  s.width = p.width;
  s.height = p.height;
  s.shardSize = p.shardSize;
  s.shardsX = p.shardsX;
  s.rank = p.rank;
  s.world = p.world;
  return s;
}
// ... with what follows from them: the share's wave tiles and slots (colStride == slots by construction)
__host__ __device__ inline void setShare(RenderParams& p, const Share& s) {
  p.width = s.width;
  p.height = s.height;
  p.shardSize = s.shardSize;
  p.shardTiles = shardTiles(s);
  p.shardsX = s.shardsX;
  p.rank = s.rank;
  p.world = s.world;
  p.numItems = waveTiles(s);
  p.colStride = (size_t)slots(s);
}

// the first pixel of the share's 8x8 wave tile `tile` (row-major inside its shard tile); lane k of
// the wave has pixel (x + (k & 7), y + (k >> 3)), which may lie outside the image. per = shardTiles(s):
// a kernel passes its parameter block's copy (setShare) rather than multiply per claimed tile
__host__ __device__ inline int2 tileOrigin(const Share& s, int tile, int per) {
  const int sub = s.shardSize >> 3;  // wave tiles per shard-tile edge
  const int j = tile / per, t = tile - j * per;
  const int g = j * s.world + s.rank;  // global shard tile id (row-major)
  const int gy = g / s.shardsX, gx = g - gy * s.shardsX;
  return make_int2(gx * s.shardSize + (t % sub) * 8, gy * s.shardSize + (t / sub) * 8);
}
__host__ __device__ inline int2 tileOrigin(const Share& s, int tile) { return tileOrigin(s, tile, shardTiles(s)); }
// slot of pixel (px, py), which must be one of the share's
__host__ __device__ inline size_t slotOf(const Share& s, int px, int py) {
  const int ss = s.shardSize;
  const int gx = px / ss, gy = py / ss;
  const int j = (gy * s.shardsX + gx) / s.world;  // the share's j-th shard tile
  return (size_t)j * ss * ss + (size_t)((py - gy * ss) * ss + (px - gx * ss));
}
// slotOf's inverse; false for a slot outside the image
__host__ __device__ inline bool pixelOfSlot(const Share& s, long k, int& px, int& py) {
  const long perTile = (long)s.shardSize * s.shardSize;
  long j = k / perTile;
  int within = (int)(k - j * perTile);
  long g = j * s.world + s.rank;
  int gy = (int)(g / s.shardsX), gx = (int)(g - (long)gy * s.shardsX);
  px = gx * s.shardSize + within % s.shardSize;
  py = gy * s.shardSize + within / s.shardSize;
  return px < s.width && py < s.height;
}

}  // namespace pt

#ifdef __HIPCC__
#include "pt_device.h"
#include "pt_trace.h"

namespace pt {

// ------------------------------------------------------------ camera ray
// main IS:846-850: the pixel's RNG seed ...
__device__ __forceinline__ uint32_t pixelSeed(int px, int py, uint32_t sampleIndex) {
  return ((uint32_t)px * 1973u + (uint32_t)py * 9277u + sampleIndex * 26699u) | 1u;
}
// ... and the ray through pixel (px, py from the bottom-left) of a W x H image, (ax, ay) off its
// centre in NDC (the AA jitter; 0 for the guide pass, whose x is then pixx + 0.0f)
__device__ __forceinline__ V3 cameraDir(const float* M, int W, int H, int px, int py, float ax, float ay) {
  float pixx = (float)(2 * px + 1) / (float)W - 1.0f;
  float pixy = (float)(2 * py + 1) / (float)H - 1.0f;
  float x = pixx + ax, y = pixy + ay, z = -1.5f;
  V3 c0 = v3(M[0], M[1], M[2]), c1 = v3(M[4], M[5], M[6]), c2 = v3(M[8], M[9], M[10]), c3 = v3(M[12], M[13], M[14]);
  V3 dir = (c0 * x + c1 * y) + (c2 * z + c3 * 0.0f);
  return normalize(dir);
}
// seed and jittered camera ray of a frame's sample of pixel (px, py); seed is left as the path needs it
__device__ __forceinline__ V3 cameraRay(const float* M, int W, int H, uint32_t sampleIndex, int px, int py,
                                        uint32_t& seed) {
  seed = pixelSeed(px, py, sampleIndex);
  float ax = (randf(seed) - 0.5f) / (float)W;
  float ay = (randf(seed) - 0.5f) / (float)H;
  return cameraDir(M, W, H, px, py, ax, ay);
}
__device__ __forceinline__ V3 cameraRay(const RenderParams& p, uint32_t sampleIndex, int px, int py, uint32_t& seed) {
  return cameraRay(p.cam, p.width, p.height, sampleIndex, px, py, seed);
}
// the path's RNG state of a ray taken as pixel (px, py)'s camera ray of that sample: cameraRay's seed after
// its two jitter draws (the radiance query, pt_radiance.hip)
__device__ __forceinline__ uint32_t pathSeed(int px, int py, uint32_t sampleIndex) {
  uint32_t seed = pixelSeed(px, py, sampleIndex);
  (void)randf(seed);
  (void)randf(seed);
  return seed;
}

// ------------------------------------------------------------ frame and store
// frame fr of the launch's batch: its sample index and colour buffer
__device__ __forceinline__ FrameRef frameRef(const RenderParams& p, int fr) {
  FrameRef f;
  f.col = p.col ? p.col + (size_t)fr * p.colStride * COL_F : nullptr;
  f.sampleIndex = p.sampleIndex + (uint32_t)fr * p.sampleStride;
  return f;
}
// the pixel's sample of frame f: into the frame's colour buffer (a pipelined frame; mixFrames updates
// the running mean in frame order) or mixed into the running mean in place (IS:868-871)
__device__ __forceinline__ void storeSample(const RenderParams& p, const FrameRef& f, int px, int py, V3 color) {
  if (f.col) {
    stCol(f.col + slotOf(shareOf(p), px, py) * COL_F, color.x, color.y, color.z);
    return;
  }
  float4* a = p.accum + (size_t)py * p.width + px;
  float4 old = ldStream(a);
  float w = 1.0f / (float)(p.frameCounter + 1u);
  stStream(a, make_float4(mixf(old.x, color.x, w), mixf(old.y, color.y, w), mixf(old.z, color.z, w), 1.0f));
}

// ------------------------------------------------------------ camera-ray bins
// The closest of a bin's n candidate triangles (fetchTri(k): candidate k's four geometry float4), each
// tested with hitTriangle's exact arithmetic (IS:251-301): best = its position in the bin (-1: none),
// tie = another candidate at exactly tbest (the caller retraces in the reference order)
template <class F>
__device__ __forceinline__ void closestInBin(int n, bool valid, V3 eye, V3 dir, F fetchTri, float& tbest, int& best,
                                             bool& tie) {
  tbest = PT_INF;
  best = -1;
  tie = false;
  for (int k = 0; k < n; k++) {
    const float4* g = fetchTri(k);
    float tt;
    const bool h = valid && triTest(g[0], g[1], g[2], g[3], eye, dir, PT_INF, tt);
    if (h && tt == tbest) tie = true;
    if (h && tt < tbest) {
      tbest = tt;
      best = k;
    }
  }
}

}  // namespace pt
#endif  // __HIPCC__
