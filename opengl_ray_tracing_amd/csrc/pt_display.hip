// pt_display.hip -- what follows a frame kernel over the pixels of a share (pt_frame.h Share, one
// lane per slot): pass3's tonemap, the pack / unpack of the multi-GPU tile gather, the 8-bit display
// forms, and the running-mean update of a batch of pipelined frames (mixFrames).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_frame.h"
#include "pt_kernels.h"

namespace pt {

// ------------------------------------------------------------ epilogues
// (tonemapPixel: pt_device.h, shared with the denoiser's colour term)
__global__ void tonemapKernel(const float4* accum, float* rgb, int n, float limit, float gamma) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 c = tonemapPixel(accum[i], limit, gamma);
  rgb[3 * i] = c.x;
  rgb[3 * i + 1] = c.y;
  rgb[3 * i + 2] = c.z;
}
hipError_t launchTonemap(const float4* accum, float* rgb, int n, float limit, float gamma, hipStream_t s) {
  hipLaunchKernelGGL(tonemapKernel, dim3((n + 255) / 256), dim3(256), 0, s, accum, rgb, n, limit, gamma);
  return hipGetLastError();
}
// pass3's fragColor as the GLUT_RGBA window stores it (OpenglRayTracing/main.cpp glutInitDisplayMode,
// an 8-bit unsigned-normalised framebuffer): round(clamp(x, 0, 1) * 255), as one fused multiply-add
// (NaN -> 0)
__device__ __forceinline__ uint32_t unorm8(float x) {
  const float c = fminf(fmaxf(x, 0.0f), 1.0f);
  return (uint32_t)__builtin_fmaf(c, 255.0f, 0.5f);
}

// packed slots are (r, g, b): the running mean's alpha is 1 for every rendered pixel
// (IS:868-871 writes vec4(color, 1)), so the gather moves 12 bytes per pixel, not 16
__global__ void packKernel(PackParams p, const float4* accum, float* packed) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  const float4 c = pixelOfSlot(p.share, k, px, py) ? accum[(size_t)py * p.share.width + px] : make_float4(0, 0, 0, 0);
  packed[3 * k] = c.x;
  packed[3 * k + 1] = c.y;
  packed[3 * k + 2] = c.z;
}
__global__ void unpackKernel(PackParams p, float4* accum, const float* packed) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (pixelOfSlot(p.share, k, px, py))
    accum[(size_t)py * p.share.width + px] = make_float4(packed[3 * k], packed[3 * k + 1], packed[3 * k + 2], 1.0f);
}
hipError_t launchPack(const PackParams& p, const float4* accum, float* packed, hipStream_t s) {
  if (p.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(packKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, packed);
  return hipGetLastError();
}
hipError_t launchUnpack(const PackParams& p, float4* accum, const float* packed, hipStream_t s) {
  if (p.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(unpackKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, packed);
  return hipGetLastError();
}

// The displayed frame (pass3 into the 8-bit window) of a screen-tile split: each rank packs its
// own tiles' display values (3 bytes per pixel, packed order) and rank 0 writes its own tiles and
// unpacks every other rank's into one RGBA8 image -- a quarter of the f32 gather's bytes over xGMI.
__global__ void displayPackKernel(PackParams p, const float4* accum, float limit, float gamma, uint8_t* packed) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  uint32_t r = 0, g = 0, b = 0;
  if (pixelOfSlot(p.share, k, px, py)) {
    const V3 c = tonemapPixel(accum[(size_t)py * p.share.width + px], limit, gamma);
    r = unorm8(c.x), g = unorm8(c.y), b = unorm8(c.z);
  }
  packed[3 * k] = (uint8_t)r;
  packed[3 * k + 1] = (uint8_t)g;
  packed[3 * k + 2] = (uint8_t)b;
}
__global__ void displayOwnKernel(PackParams p, const float4* accum, float limit, float gamma, uchar4* image) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (!pixelOfSlot(p.share, k, px, py)) return;
  const size_t i = (size_t)py * p.share.width + px;
  const V3 c = tonemapPixel(accum[i], limit, gamma);
  image[i] = make_uchar4((uint8_t)unorm8(c.x), (uint8_t)unorm8(c.y), (uint8_t)unorm8(c.z), 255);
}
hipError_t launchDisplayPack(const PackParams& p, const float4* accum, float limit, float gamma, uint8_t* packed,
                             hipStream_t s) {
  if (p.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(displayPackKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, limit,
                     gamma, packed);
  return hipGetLastError();
}
hipError_t launchDisplayOwn(const PackParams& p, const float4* accum, float limit, float gamma, uchar4* image,
                            hipStream_t s) {
  if (p.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(displayOwnKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, limit,
                     gamma, image);
  return hipGetLastError();
}
// blockIdx.y = rank - 1 of ranks 1..world-1 (their packed buffers in d.src)
__global__ void displayUnpackKernel(RanksUnpack d, uchar4* image) {
  const int rank = blockIdx.y + 1;
  const uint8_t* src = static_cast<const uint8_t*>(d.src[rank]);
  if (!src) return;
  PackParams p = d.base;
  p.share.rank = rank;
  p.count = d.count[rank];
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (pixelOfSlot(p.share, k, px, py))
    image[(size_t)py * p.share.width + px] = make_uchar4(src[3 * k], src[3 * k + 1], src[3 * k + 2], 255);
}
hipError_t launchDisplayUnpack(const RanksUnpack& d, int world, uchar4* image, hipStream_t s) {
  long most = 0;
  for (int k = 1; k < world; k++) most = d.count[k] > most ? d.count[k] : most;
  if (world < 2 || most <= 0) return hipSuccess;
  hipLaunchKernelGGL(displayUnpackKernel, dim3((unsigned)((most + 255) / 256), (unsigned)(world - 1)), dim3(256), 0, s,
                     d, image);
  return hipGetLastError();
}

// unpackKernel of ranks 1..world-1 in one launch (blockIdx.y = rank - 1): rank 0's reassembly of
// a gather of the f32 running means after each batch of frames
__global__ void unpackRanksKernel(RanksUnpack d, float4* accum) {
  const int rank = blockIdx.y + 1;
  const float* src = static_cast<const float*>(d.src[rank]);
  if (!src) return;
  PackParams p = d.base;
  p.share.rank = rank;
  p.count = d.count[rank];
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (pixelOfSlot(p.share, k, px, py))
    accum[(size_t)py * p.share.width + px] = make_float4(src[3 * k], src[3 * k + 1], src[3 * k + 2], 1.0f);
}
hipError_t launchUnpackRanks(const RanksUnpack& d, int world, float4* accum, hipStream_t s) {
  long most = 0;
  for (int k = 1; k < world; k++) most = d.count[k] > most ? d.count[k] : most;
  if (world < 2 || most <= 0) return hipSuccess;
  hipLaunchKernelGGL(unpackRanksKernel, dim3((unsigned)((most + 255) / 256), (unsigned)(world - 1)), dim3(256), 0, s,
                     d, accum);
  return hipGetLastError();
}

// The gather of a PT_FLAG_SHARE_MOMENTS split: packKernel / unpackRanksKernel with the pixel's moments
// behind its colour, PACK_STATS_F = 5 floats (r, g, b, m1, m2), 20 bytes per slot. One lane per slot;
// the accumulation (16 B) and the moments (8 B) are touched once per gather, so they stream like the
// running-mean update's. The packed side is written as the 12-byte pack writes it, one dword store per
// float and lane: a slot's 20 bytes are 4-byte aligned only, and a wave's five stores together cover
// 1280 contiguous bytes. (Staging a block's slots through LDS would make each store instruction
// contiguous; not done: the 12-byte pack has not needed it.) The packed buffers themselves are plain
// accesses: the collective reads what the pack wrote, and the unpack what the collective wrote.
__global__ void packStatsKernel(PackParams p, const float4* accum, const float2* moments, float* packed) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  float4 c = make_float4(0, 0, 0, 0);
  float2 m = make_float2(0, 0);
  if (pixelOfSlot(p.share, k, px, py)) {
    const size_t i = (size_t)py * p.share.width + px;
    c = ldStream(accum + i);
    m = ldStream(moments + i);
  }
  float* out = packed + PACK_STATS_F * k;
  out[0] = c.x;
  out[1] = c.y;
  out[2] = c.z;
  out[3] = m.x;
  out[4] = m.y;
}
hipError_t launchPackStats(const PackParams& p, const float4* accum, const float2* moments, float* packed,
                           hipStream_t s) {
  if (!accum || !moments || !packed) return hipErrorInvalidValue;
  if (p.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(packStatsKernel, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, moments,
                     packed);
  return hipGetLastError();
}
// blockIdx.y = rank - 1 of ranks 1..world-1, as unpackRanksKernel
__global__ void unpackRanksStatsKernel(RanksUnpack d, float4* accum, float2* moments) {
  const int rank = blockIdx.y + 1;
  const float* src = static_cast<const float*>(d.src[rank]);
  if (!src) return;
  PackParams p = d.base;
  p.share.rank = rank;
  p.count = d.count[rank];
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  int px, py;
  if (!pixelOfSlot(p.share, k, px, py)) return;
  const float* in = src + PACK_STATS_F * k;
  const size_t i = (size_t)py * p.share.width + px;
  stStream(accum + i, make_float4(in[0], in[1], in[2], 1.0f));
  stStream(moments + i, make_float2(in[3], in[4]));
}
hipError_t launchUnpackRanksStats(const RanksUnpack& d, int world, float4* accum, float2* moments, hipStream_t s) {
  if (!accum || !moments) return hipErrorInvalidValue;
  long most = 0;
  for (int k = 1; k < world; k++) most = d.count[k] > most ? d.count[k] : most;
  if (world < 2 || most <= 0) return hipSuccess;
  hipLaunchKernelGGL(unpackRanksStatsKernel, dim3((unsigned)((most + 255) / 256), (unsigned)(world - 1)), dim3(256), 0,
                     s, d, accum, moments);
  return hipGetLastError();
}

// The running means of a batch of pipelined frames (storeSample's update, deferred to frame order):
// frame f's colours at col + f * colStride, slot k of the share (pt_frame.h slotOf), its weight
// 1 / (frameCounter + f + 1); the pixel's mean after each frame is the one serial frames store (mixf
// of the same floats).
// MOMENTS (a PT_FLAG_MOMENTS context, pt_abi.h): plus the running means of the sample luminance l and
// of l * l, kept per pixel in a float2 plane (m1, m2) -- the same loop, the same weights and the same
// mixf as the colour, so the accumulation equals a plain context's bit for bit.
// tests/variance_ref.py (moments_update) is the specification: l = (0.3 r + 0.6 g) + 0.1 b is
// tonemapPixel's luminance, one f32 operation each (no fused multiply-add).
// Per pixel and launch: 32 B of accumulation and 16 B of moments (read + written once each, streaming
// like the accumulation) and 12 B per frame of sample colour.
// ADAPTIVE (a PT_FLAG_ADAPTIVE context, pt_adaptive.hip): a pixel whose 8x8 tile has retired
// (retiredAt[ty * tilesX + tx] != 0) keeps its accumulation and moments -- the camera-ray pass stored it
// no sample -- and returns before its loads; every other pixel is a MOMENTS pixel.
// SKY (pt_kernels.h SkyTiles; the launch's camera-ray pass ran over its pass list): a pixel whose image
// tile has an empty camera-ray bin was not given to the pass. Its sample of frame f is the sky's along its
// camera ray, sampleHdr(env, cameraRay(cam, W, H, sampleIndex + f * sampleStride, px, py)) -- the functions
// and the floats of the pass (pt_frame.h, pt_device.h), so the means are bit for bit what they were -- and
// the update counts those rays, one atomic per wave. A retired tile (ADAPTIVE) takes no sample and counts
// none, as in the pass. The frames' texel lookups are independent: they are taken SKY_CHUNK at a time, the
// indices first and then the loads, so a chunk's loads are in flight together.
// SKY is a template parameter: without it the kernels are the 16-20 VGPR streaming updates they were (the
// lookups take 58-64), which find room beside a machine full of regen blocks sooner -- what the launches
// without such tiles (no pass, no bins, the large scenes) keep.
constexpr int SKY_CHUNK = 4;
template <bool MOMENTS, bool ADAPTIVE, bool SKY>
__device__ __forceinline__ void mixFrames(const PackParams& p, float4* accum, float2* moments, const float* col,
                                          size_t colStride, int nFrames, uint32_t frameCounter, const SkyTiles& sky,
                                          const uint32_t* retiredAt) {
  long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
  int px = 0, py = 0;
  bool on = k < p.count && pixelOfSlot(p.share, k, px, py);
  if (ADAPTIVE && on && retiredAt[(size_t)(py >> 3) * ((p.share.width + 7) >> 3) + (px >> 3)] != 0u) on = false;
  bool own = false;  // the update takes this pixel's samples itself
  if (SKY) {
    if (on) {
      const int t = (py >> 3) * sky.binTilesX + (px >> 3);
      own = sky.binStart[t + 1] == sky.binStart[t];
    }
    // the rays the pass counted for these pixels: one per valid pixel and frame
    const unsigned long long b = __ballot(own);
    if ((threadIdx.x & 63) == 0 && b)
      atomicAdd(sky.rayShards + (blockIdx.x & (RAY_SHARDS - 1)) * RAY_SHARD_STRIDE,
                (unsigned long long)__popcll(b) * (unsigned long long)nFrames);
  }
  if (!on) return;
  const size_t i = (size_t)py * p.share.width + px;
  float4 a = ldStream(accum + i);
  float2 m = make_float2(0.0f, 0.0f);
  if (MOMENTS) m = ldStream(moments + i);
  auto mix = [&](int f, float cx, float cy, float cz) {
    const float w = 1.0f / (float)(frameCounter + (uint32_t)f + 1u);
    a = make_float4(mixf(a.x, cx, w), mixf(a.y, cy, w), mixf(a.z, cz, w), 1.0f);
    if (MOMENTS) {
      const float l = (0.3f * cx + 0.6f * cy) + 0.1f * cz;
      m = make_float2(mixf(m.x, l, w), mixf(m.y, l * l, w));
    }
  };
  if (!SKY || !own) {
    for (int f = 0; f < nFrames; f++) {
      const float3 c = ldCol(col + ((size_t)f * colStride + k) * COL_F);
      mix(f, c.x, c.y, c.z);
    }
  } else if (!sky.env.hdr) {  // no environment: sampleHdr's black
    for (int f = 0; f < nFrames; f++) mix(f, 0.0f, 0.0f, 0.0f);
  } else {
    for (int f0 = 0; f0 < nFrames; f0 += SKY_CHUNK) {
      int tex[SKY_CHUNK];
#pragma unroll
      for (int j = 0; j < SKY_CHUNK; j++) {  // (past the batch's end: its last frame's again, not mixed)
        const int f = min(f0 + j, nFrames - 1);
        uint32_t seed;
        const V3 dir = cameraRay(sky.cam, p.share.width, p.share.height, sky.sampleIndex + (uint32_t)f * sky.sampleStride,
                                 px, py, seed);
        tex[j] = sampleHdrTexel(sky.env, dir);
      }
      V3 c[SKY_CHUNK];
      sampleHdrAt(sky.env, tex, c);
#pragma unroll
      for (int j = 0; j < SKY_CHUNK; j++)
        if (f0 + j < nFrames) mix(f0 + j, c[j].x, c[j].y, c[j].z);
    }
  }
  stStream(accum + i, a);
  if (MOMENTS) stStream(moments + i, m);
}
template <bool SKY>
__global__ void mixKernel(PackParams p, float4* accum, const float* col, size_t colStride, int nFrames,
                          uint32_t frameCounter, SkyTiles sky) {
  mixFrames<false, false, SKY>(p, accum, nullptr, col, colStride, nFrames, frameCounter, sky, nullptr);
}
template <bool SKY>
__global__ void mixMomentsKernel(PackParams p, float4* accum, float2* moments, const float* col, size_t colStride,
                                 int nFrames, uint32_t frameCounter, SkyTiles sky) {
  mixFrames<true, false, SKY>(p, accum, moments, col, colStride, nFrames, frameCounter, sky, nullptr);
}
template <bool SKY>
__global__ void mixAdaptiveKernel(PackParams p, float4* accum, float2* moments, const float* col, size_t colStride,
                                  int nFrames, uint32_t frameCounter, const uint32_t* retiredAt, SkyTiles sky) {
  mixFrames<true, true, SKY>(p, accum, moments, col, colStride, nFrames, frameCounter, sky, retiredAt);
}
hipError_t launchMix(const PackParams& p, float4* accum, const float* col, size_t colStride, int nFrames,
                     uint32_t frameCounter, const SkyTiles& sky, hipStream_t s) {
  if (sky.binStart && !sky.rayShards) return hipErrorInvalidValue;
  if (p.count <= 0 || nFrames <= 0) return hipSuccess;
  hipLaunchKernelGGL(sky.binStart ? mixKernel<true> : mixKernel<false>, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, col, colStride,
                     nFrames, frameCounter, sky);
  return hipGetLastError();
}
hipError_t launchMixMoments(const PackParams& p, float4* accum, float2* moments, const float* col, size_t colStride,
                            int nFrames, uint32_t frameCounter, const SkyTiles& sky, hipStream_t s) {
  if (sky.binStart && !sky.rayShards) return hipErrorInvalidValue;
  if (p.count <= 0 || nFrames <= 0) return hipSuccess;
  hipLaunchKernelGGL(sky.binStart ? mixMomentsKernel<true> : mixMomentsKernel<false>, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, moments, col,
                     colStride, nFrames, frameCounter, sky);
  return hipGetLastError();
}
hipError_t launchMixAdaptive(const PackParams& p, float4* accum, float2* moments, const float* col, size_t colStride,
                             int nFrames, uint32_t frameCounter, const uint32_t* retiredAt, const SkyTiles& sky,
                             hipStream_t s) {
  if (!retiredAt || (sky.binStart && !sky.rayShards)) return hipErrorInvalidValue;
  if (p.count <= 0 || nFrames <= 0) return hipSuccess;
  hipLaunchKernelGGL(sky.binStart ? mixAdaptiveKernel<true> : mixAdaptiveKernel<false>, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p, accum, moments,
                     col, colStride, nFrames, frameCounter, retiredAt, sky);
  return hipGetLastError();
}

}  // namespace pt
