// pt_variance.hip -- the variance estimate and the variance-guided a-trous filter (pt_abi.h
// pt_denoise_var; Schied et al. 2017, the spatial part): pt_denoise.hip's filter with its colour
// term replaced by a luminance term scaled by each pixel's estimated standard deviation, and the
// variance propagated from pass to pass. tests/variance_ref.py is the specification: every f32
// operation below is one of its operations, in its order, so the output equals it bit for bit (no
// fused multiply-adds, IEEE division and square root, ptm_expf shared with the host).
//
//  * varLumKernel: l = lum(tm(c)) of the input, one float per pixel.
//  * varInitKernel (step A): the initial variance from the context's sample moments, or from the
//    7 x 7 window of l when there are none (yet); writes it twice, as the plane pt_download_variance
//    returns and beside l in the first pass's (l, v) plane.
//  * atrousVarKernel (step B), one launch per pass: pt_atrous.h's tile function with the
//    luminance/variance term below. A tap needs 15 floats and a flag: colour, l, v, position,
//    normal, albedo. l and v travel in a float2 plane that each pass writes beside its colour for
//    the next one, so a tap never recomputes the tonemap. Per pixel a pass reads 16 + 8 + 48 B of 25
//    taps (pt_denoise: 80 B), 9 taps of the 3 x 3 variance prefilter around the centre, and writes
//    16 + 8 B. Staged, a pixel's four float4 are (c.rgb, valid), (P.xyz, l), (N.xyz, v), (A.rgb, -);
//    the prefilter reads the same tile (halo >= 2 >= 1). A tap outside the image or on a miss pixel
//    adds variance 0, as it adds colour 0.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_atrous.h"
#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

__device__ __forceinline__ float lum3(float r, float g, float b) { return (0.3f * r + 0.6f * g) + 0.1f * b; }
__device__ __forceinline__ float lumTm(float4 c, float limit) {
  const V3 t = tonemapPixel(c, limit, 0.0f);
  return lum3(t.x, t.y, t.z);
}
// the .w of a float4 plane's pixel, a 4-byte load
__device__ __forceinline__ bool hitAt(const float4* nrmTri, size_t g) {
  return __float_as_int(reinterpret_cast<const float*>(nrmTri + g)[3]) >= 0;
}

__global__ void varLumKernel(const float4* in, float* lum, int n, float limit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lum[i] = lumTm(in[i], limit);
}

__global__ __launch_bounds__(ATROUS_TILE* ATROUS_TILE) void varInitKernel(VarInitParams p) {
  const int W = p.width, H = p.height;
  const int px = blockIdx.x * ATROUS_TILE + (threadIdx.x & (ATROUS_TILE - 1));
  const int py = blockIdx.y * ATROUS_TILE + threadIdx.x / ATROUS_TILE;
  if (px >= W || py >= H) return;
  const size_t i = (size_t)py * W + px;
  float v = 0.0f;
  if (hitAt(p.nrmTri, i)) {
    if (p.moments) {
      const float4 c = p.in[i];
      const float2 m = p.moments[i];
      const float L = lum3(c.x, c.y, c.z);
      const float q = 1.0f + L / p.limit;
      const float gd = 1.0f / (q * q);
      const float n = c.w > p.kf ? c.w : p.kf;
      float d = m.y - m.x * m.x;
      d = d > 0.0f ? d : 0.0f;
      v = (d / n) * (gd * gd);
    } else {
      float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
      for (int dy = -3; dy <= 3; dy++) {
        const int qy = py + dy;
        const int cy = min(max(qy, 0), H - 1);
#pragma unroll
        for (int dx = -3; dx <= 3; dx++) {
          const int qx = px + dx;
          const int cx = min(max(qx, 0), W - 1);  // the load stays in the image
          const size_t g = (size_t)cy * W + cx;
          const bool valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & hitAt(p.nrmTri, g);
          const float lq = valid ? p.lum[g] : 0.0f;
          s1 = s1 + lq;
          s2 = s2 + lq * lq;
          cnt = cnt + (valid ? 1.0f : 0.0f);
        }
      }
      const float mu = s1 / cnt;
      const float d = s2 / cnt - mu * mu;
      v = d > 0.0f ? d : 0.0f;
    }
  }
  p.var0[i] = v;
  p.lv[i] = make_float2(p.lum[i], v);
}

// the luminance term |l(q) - l(p)| / (sigma_l * sqrt(3 x 3 mean of v around p) + 1e-6), and the
// variance filtered beside the colour with the squared weights
struct VarianceTerm {
  using Params = AtrousVarParams;
  using Px = float2;  // (l, v)
  static __device__ __forceinline__ Px load(const Params& p, size_t g) { return p.lvIn[g]; }
  static __device__ __forceinline__ void pack(float4 pos, float4 nrm, float4 alb, Px lv, float4& b, float4& c,
                                              float4& d) {
    b = make_float4(pos.x, pos.y, pos.z, lv.x);
    c = make_float4(nrm.x, nrm.y, nrm.z, lv.y);
    d = make_float4(alb.x, alb.y, alb.z, 0.0f);
  }
  static __device__ __forceinline__ void unpack(float4 b, float4 c, float4 d, V3& P, V3& N, V3& A, Px& lv) {
    P = v3(b.x, b.y, b.z);
    N = v3(c.x, c.y, c.z);
    A = v3(d.x, d.y, d.z);
    lv = make_float2(b.w, c.w);
  }

  const size_t i;
  const float2 lvP;
  float vOut;
  bool lOn;
  float lden = 1.0f, svar = 0.0f;
  __device__ __forceinline__ VarianceTerm(const Params& p, size_t i_) : i(i_), lvP(p.lvIn[i_]), vOut(lvP.y) {}
  // the luminance term's scale: the 3 x 3 mean of v around the centre
  template <bool STAGE>
  __device__ __forceinline__ void centre(const Params& p, const AtrousAt& at, const float4* s_px) {
    lOn = p.sigmaL > 0.0f;
    if (!lOn) return;
    const int W = at.W, H = at.H, R = at.R;
    float sg = 0.0f, sv = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);  // exact in f32
        float vq;
        bool valid;
        if (STAGE) {
          const int li = (at.ly + 2 * at.s + dy) * R + (at.lx + 2 * at.s + dx);
          valid = __float_as_int(s_px[li].w) != 0;
          vq = s_px[2 * R * R + li].w;
        } else {
          const int qx = at.px + dx, qy = at.py + dy;
          const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);  // the load stays in the image
          const size_t gi = (size_t)cy * W + cx;
          valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & hitAt(p.nrmTri, gi);
          vq = p.lvIn[gi].y;
        }
        const float gq = valid ? g : 0.0f;
        vq = valid ? vq : 0.0f;
        sg = sg + gq;
        sv = sv + vq * gq;
      }
    }
    lden = p.sigmaL * sqrtf(sv / sg) + 1e-6f;
  }
  __device__ __forceinline__ void range(const Params&, Px lv, float& a) const {
    if (lOn) a = a + fabsf(lv.x - lvP.x) / lden;
  }
  __device__ __forceinline__ void accumulate(bool valid, Px lv, float w) {
    const float vq = valid ? lv.y : 0.0f;
    svar = svar + vq * (w * w);
  }
  __device__ __forceinline__ void normalise(float sw) { vOut = svar / (sw * sw); }
  // a miss pixel's colour is copied, so is its l
  __device__ __forceinline__ void write(const Params& p, float4 out, bool hit) const {
    if (p.lvOut) p.lvOut[i] = make_float2(hit ? lumTm(out, p.limit) : lvP.x, vOut);
  }
};

template <bool STAGE>
__global__ __launch_bounds__(ATROUS_TILE* ATROUS_TILE) void atrousVarKernel(AtrousVarParams p) {
  extern __shared__ __attribute__((aligned(16))) float4 s_px[];
  atrousTile<VarianceTerm, STAGE>(p, s_px);
}

hipError_t launchVarLum(const float4* in, float* lum, int n, float limit, hipStream_t s) {
  hipLaunchKernelGGL(varLumKernel, dim3((n + 255) / 256), dim3(256), 0, s, in, lum, n, limit);
  return hipGetLastError();
}

hipError_t launchVarInit(const VarInitParams& p, hipStream_t s) {
  const dim3 grid((p.width + ATROUS_TILE - 1) / ATROUS_TILE, (p.height + ATROUS_TILE - 1) / ATROUS_TILE);
  hipLaunchKernelGGL(varInitKernel, grid, dim3(ATROUS_TILE * ATROUS_TILE), 0, s, p);
  return hipGetLastError();
}

hipError_t launchAtrousVar(const AtrousVarParams& p, hipStream_t s) {
  return launchAtrousPass(atrousVarKernel<true>, atrousVarKernel<false>, p, s);
}

}  // namespace pt
