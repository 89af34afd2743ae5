// pt_adaptive.hip -- adaptive sampling's decision (pt_abi.h pt_adaptive_update): which 8x8 tiles of
// the image have converged and retire. tests/adaptive_ref.py is the specification: every f32
// operation below is one of its operations, in its order, so err2 and retiredAt equal it bit for bit
// (no fused multiply-adds, IEEE division).
//
// tileErrorKernel: one wave per 8x8 wave tile of the context's share (pt_frame.h tileOrigin: a shard
// tile's edge is a multiple of 8, so a wave tile is one whole tile of the image and belongs to this
// rank alone), one lane per pixel; with world 1 that is every tile of the image, in shard order -- a
// tile's result does not depend on the order. A wave tile outside the image returns at once; entries
// of other ranks' tiles are never written (they stay 0: active, which is harmless -- this rank renders
// none of their pixels). A retired tile's wave returns after one scalar load (the tile index is
// wave-uniform). An active tile's lanes read their pixel's
// accumulation (16 B) and moments (8 B), streaming -- nothing here reads them twice -- and form the
// variance of the mean of the tone-mapped luminance, pt_denoise_var's step A from the moments with
// n_p = kf and no guides; the wave takes the largest (all are >= 0 or NaN, and a NaN never wins the
// select, so the order of the butterfly does not matter) and lane 0 stores the tile's two words.
// At 1080p, world 1: 32 640 waves (240 of them outside the image) and about 50 MB read with every
// tile active; a 1/N share launches 1/N of the waves.
#include "pt_device.h"
#include "pt_frame.h"

namespace pt {

constexpr int TILE_ERR_BS = 256;  // four tiles per block

__global__ __launch_bounds__(TILE_ERR_BS) void tileErrorKernel(TileErrorParams p) {
  const int lane = threadIdx.x & 63;
  const int t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TILE_ERR_BS / 64) + (threadIdx.x >> 6)));
  if (t >= p.waveTiles) return;
  const int2 o = tileOrigin(p.share, t, p.shardTiles);
  if (o.x >= p.share.width || o.y >= p.share.height) return;  // a shard tile's part outside the image
  const int T = (o.y >> 3) * p.tilesX + (o.x >> 3);
  if (p.retiredAt[T] != 0u) return;  // keeps its err2 and retiredAt
  const int px = o.x + (lane & 7), py = o.y + (lane >> 3);
  float e = 0.0f;
  if (px < p.share.width && py < p.share.height) {
    const size_t i = (size_t)py * p.share.width + px;
    const float4 c = ldStream(p.accum + i);
    const float2 m = ldStream(p.moments + i);
    const float L = (0.3f * c.x + 0.6f * c.y) + 0.1f * c.z;
    const float q = 1.0f + L / p.limit;
    const float gd = 1.0f / (q * q);
    float d = m.y - m.x * m.x;
    d = d > 0.0f ? d : 0.0f;
    const float v = (d / p.kf) * (gd * gd);
    e = v > e ? v : e;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float x = __shfl_xor(e, o);
    e = x > e ? x : e;
  }
  if (lane == 0) {
    p.err2[T] = e;
    if (p.frames >= (uint32_t)p.minFrames && e <= p.thr2) p.retiredAt[T] = p.frames;
  }
}

hipError_t launchTileError(const TileErrorParams& p, hipStream_t s) {
  if (!p.accum || !p.moments || !p.err2 || !p.retiredAt || p.waveTiles < 0 || p.tilesX <= 0 || p.shardTiles <= 0)
    return hipErrorInvalidValue;
  if (p.waveTiles == 0) return hipSuccess;  // a rank past the last shard tile: nothing to decide
  const int perBlock = TILE_ERR_BS / 64;
  hipLaunchKernelGGL(tileErrorKernel, dim3((unsigned)((p.waveTiles + perBlock - 1) / perBlock)), dim3(TILE_ERR_BS), 0, s, p);
  return hipGetLastError();
}

}  // namespace pt
