// pt_temporal.hip -- the temporal resolve (pt_abi.h pt_temporal_resolve): the running mean of the
// current camera blended with the previous camera's resolved image, which is fetched through the
// first-hit position the guide buffers hold for every pixel. The scene is static, so that
// position projects straight into the previous camera: no ray is traced. tests/temporal_ref.py is
// the specification: every f32 operation below is one of its operations, in its order, so the
// output equals it bit for bit (no fused multiply-adds, IEEE division, no transcendental).
//
// One lane per pixel; a block is a 16 x 16 tile and each of its four waves an 8 x 8 quadrant, so
// a wave's centre loads are eight 128-byte rows per plane and its 2 x 2 history gathers stay
// within a few lines around the quadrant's projection. Per pixel: 3 float4 centre loads, 4 taps of
// 3 float4 each, 1 float4 store -- compulsory 112 B (6 planes read, 1 written), the taps of
// neighbouring lanes share their lines. Everything that depends only on the centre is hoisted;
// the tap loop has no branch: a tap outside the history image, on a history miss, without
// samples or off the centre's plane / normal gets weight 0 and colour 0 by select (the
// restatement does the same: adding +0 is exact). A tap's address is clamped into the image
// before the load.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

__global__ __launch_bounds__(TEMPORAL_TILE* TEMPORAL_TILE) void temporalKernel(TemporalParams p) {
  const int W = p.width, H = p.height;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = blockIdx.x * TEMPORAL_TILE + (wave & 1) * 8 + (lane & 7);
  const int py = blockIdx.y * TEMPORAL_TILE + (wave >> 1) * 8 + (lane >> 3);
  if (px >= W || py >= H) return;
  const size_t i = (size_t)py * W + px;
  const float4 c = p.accum[i];
  const float kf = p.frames;
  float4 out = make_float4(c.x, c.y, c.z, kf);
  if (p.hist) {
    const float4 nrmP = p.nrmTri[i];
    if (__float_as_int(nrmP.w) >= 0) {
      const float4 posP = p.posT[i];
      const V3 Pp = v3(posP.x, posP.y, posP.z), Np = v3(nrmP.x, nrmP.y, nrmP.z);
      // the centre's position in the history camera: the inverse of the camera ray (pt_frame.h cameraDir)
      const V3 v = Pp - v3(p.eye[0], p.eye[1], p.eye[2]);
      const float a = dot(v3(p.c0[0], p.c0[1], p.c0[2]), v);
      const float b = dot(v3(p.c1[0], p.c1[1], p.c1[2]), v);
      const float cz = dot(v3(p.c2[0], p.c2[1], p.c2[2]), v);
      const float s = -1.5f / cz;
      const float x = a * s, y = b * s;
      const float fW = (float)W, fH = (float)H;
      const float fx = (x + 1.0f) * (0.5f * fW) - 0.5f;
      const float fy = (y + 1.0f) * (0.5f * fH) - 0.5f;
      const bool ok = cz < 0.0f && fx > -1.0f && fx < fW && fy > -1.0f && fy < fH;  // false for NaN
      const float gx = ok ? fx : 0.0f, gy = ok ? fy : 0.0f;  // the int conversions stay defined
      const float flx = floorf(gx), fly = floorf(gy);
      const int ix = (int)flx, iy = (int)fly;
      const float tx = gx - flx, ty = gy - fly;
      const float zt = p.sigmaZ * posP.w;
      float sw = 0.0f, sn = 0.0f;
      V3 sum = v3(0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const float wy = j ? ty : 1.0f - ty;
        const int qy = iy + j;
        const int cy = min(max(qy, 0), H - 1);
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const float wt = (k ? tx : 1.0f - tx) * wy;
          const int qx = ix + k;
          const int cx = min(max(qx, 0), W - 1);  // the load stays in the image
          const size_t g = (size_t)cy * W + cx;
          const float4 hq = p.hist[g], posQ = p.histPosT[g], nrmQ = p.histNrmTri[g];
          const V3 D = v3(posQ.x, posQ.y, posQ.z) - Pp;
          // every test is evaluated (&, not &&): a reject is a select, not a branch
          const bool valid = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (__float_as_int(nrmQ.w) >= 0) &
                             (hq.w > 0.0f) & (fabsf(dot(Np, D)) <= zt) &
                             (dot(Np, v3(nrmQ.x, nrmQ.y, nrmQ.z)) >= p.normalCos);
          const float wv = valid ? wt : 0.0f;
          const V3 hc = valid ? v3(hq.x, hq.y, hq.z) : v3(0.0f, 0.0f, 0.0f);
          const float hn = valid ? hq.w : 0.0f;
          sw = sw + wv;
          sum = sum + hc * wv;
          sn = sn + hn * wv;
        }
      }
      if (ok && sw > 0.0f) {
        const V3 hc = sum / sw;
        float n = sn / sw;
        n = n < p.maxHistory ? n : p.maxHistory;
        const float wgt = kf / (n + kf);
        const float wh = 1.0f - wgt;
        out = make_float4(hc.x * wh + c.x * wgt, hc.y * wh + c.y * wgt, hc.z * wh + c.z * wgt, n + kf);
      }
    }
  }
  p.out[i] = out;
}

hipError_t launchTemporal(const TemporalParams& p, hipStream_t s) {
  const dim3 grid((p.width + TEMPORAL_TILE - 1) / TEMPORAL_TILE, (p.height + TEMPORAL_TILE - 1) / TEMPORAL_TILE);
  hipLaunchKernelGGL(temporalKernel, grid, dim3(TEMPORAL_TILE * TEMPORAL_TILE), 0, s, p);
  return hipGetLastError();
}

}  // namespace pt
