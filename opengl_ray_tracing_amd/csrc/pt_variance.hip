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
//  * atrousVarKernel (step B), one launch per pass, a block filters a 16 x 16 tile, one lane per
//    pixel. A tap needs 15 floats and a flag: colour, l, v, position, normal, albedo. l and v travel
//    in a float2 plane that each pass writes beside its colour for the next one, so a tap never
//    recomputes the tonemap. Per pixel a pass reads 16 + 8 + 48 B of 25 taps (pt_denoise: 80 B), 9 taps
//    of the 3 x 3 variance prefilter around the centre, and writes 16 + 8 B.
//    - stride <= ATROUS_LDS_STRIDE: the tile and its 2 x stride halo are staged in LDS as four float4
//      per pixel -- (c.rgb, valid), (P.xyz, l), (N.xyz, v), (A.rgb, -) -- pt_denoise's 25.6 KB at
//      stride 1 and 36.9 KB at stride 2; the prefilter reads the same tile (halo >= 2 >= 1).
//    - larger strides: direct loads, each address clamped into the image first.
//    The tap loop has no divergent branch: a tap outside the image or on a miss pixel gets w = 0,
//    colour 0 and variance 0 by select (the restatement does the same: adding +0 is exact).
#include <hip/hip_runtime.h>

#include <stdint.h>

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

// one tap's data
struct VarTapPx {
  V3 c, P, N, A;
  float l, v;
  bool valid;
};

template <bool STAGE>
__global__ __launch_bounds__(ATROUS_TILE* ATROUS_TILE) void atrousVarKernel(AtrousVarParams p) {
  extern __shared__ __attribute__((aligned(16))) float4 s_px[];  // STAGE: 4 planes of R x R pixels
  const int W = p.width, H = p.height, s = p.stride;
  const int lx = threadIdx.x & (ATROUS_TILE - 1), ly = threadIdx.x / ATROUS_TILE;
  const int x0 = blockIdx.x * ATROUS_TILE, y0 = blockIdx.y * ATROUS_TILE;
  const int px = x0 + lx, py = y0 + ly;
  const int R = ATROUS_TILE + 4 * s;  // STAGE: staged edge
  if (STAGE) {
    float4* f0 = s_px;
    float4* f1 = s_px + R * R;
    float4* f2 = s_px + 2 * R * R;
    float4* f3 = s_px + 3 * R * R;
    for (int k = threadIdx.x; k < R * R; k += ATROUS_TILE * ATROUS_TILE) {
      const int ry = k / R, rx = k - ry * R;
      const int gx = x0 - 2 * s + rx, gy = y0 - 2 * s + ry;
      float4 a = make_float4(0, 0, 0, 0), b = a, c = a, d = a;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        const size_t g = (size_t)gy * W + gx;
        const float4 col = p.in[g], pos = p.posT[g], nrm = p.nrmTri[g], alb = p.albedo[g];
        const float2 lv = p.lvIn[g];
        a = make_float4(col.x, col.y, col.z, __int_as_float(__float_as_int(nrm.w) >= 0 ? 1 : 0));
        b = make_float4(pos.x, pos.y, pos.z, lv.x);
        c = make_float4(nrm.x, nrm.y, nrm.z, lv.y);
        d = make_float4(alb.x, alb.y, alb.z, 0.0f);
      }
      f0[k] = a;
      f1[k] = b;
      f2[k] = c;
      f3[k] = d;
    }
    __syncthreads();
  }
  if (px >= W || py >= H) return;
  const size_t i = (size_t)py * W + px;
  // the centre
  const float4 cp = p.in[i];
  const float4 nrmP = p.nrmTri[i];
  const float2 lvP = p.lvIn[i];
  float4 out = cp;
  float vOut = lvP.y;
  const bool hitP = __float_as_int(nrmP.w) >= 0;
  if (hitP) {
    const float4 posP = p.posT[i], albP = p.albedo[i];
    const V3 Pp = v3(posP.x, posP.y, posP.z), Np = v3(nrmP.x, nrmP.y, nrmP.z), Ap = v3(albP.x, albP.y, albP.z);
    const float zden = p.sigmaZ * posP.w;
    const bool zOn = p.sigmaZ > 0.0f, lOn = p.sigmaL > 0.0f, aOn = p.albOn != 0;
    const int nl = p.normalLog2;
    // the luminance term's scale: the 3 x 3 mean of v around the centre
    float lden = 1.0f;
    if (lOn) {
      float sg = 0.0f, sv = 0.0f;
#pragma unroll
      for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
          const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);  // exact in f32
          float vq;
          bool valid;
          if (STAGE) {
            const int li = (ly + 2 * s + dy) * R + (lx + 2 * s + dx);
            valid = __float_as_int(s_px[li].w) != 0;
            vq = s_px[2 * R * R + li].w;
          } else {
            const int qx = px + dx, qy = py + dy;
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
    float sw = 0.0f, svar = 0.0f;
    V3 sum = v3(0.0f, 0.0f, 0.0f);
    for (int dy = -2; dy <= 2; dy++) {
      const int ady = dy < 0 ? -dy : dy;
      const float hy = ady == 0 ? 0.375f : (ady == 1 ? 0.25f : 0.0625f);
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int adx = dx < 0 ? -dx : dx;
        const float hx = adx == 0 ? 0.375f : (adx == 1 ? 0.25f : 0.0625f);
        const float k = hx * hy;  // exact in f32
        VarTapPx q;
        if (STAGE) {
          const int li = (ly + 2 * s + s * dy) * R + (lx + 2 * s + s * dx);
          const float4 a = s_px[li], b = s_px[R * R + li], c = s_px[2 * R * R + li], d = s_px[3 * R * R + li];
          q.c = v3(a.x, a.y, a.z);
          q.valid = __float_as_int(a.w) != 0;
          q.P = v3(b.x, b.y, b.z);
          q.l = b.w;
          q.N = v3(c.x, c.y, c.z);
          q.v = c.w;
          q.A = v3(d.x, d.y, d.z);
        } else {
          const int qx = px + s * dx, qy = py + s * dy;
          const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
          const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);  // the load stays in the image
          const size_t g = (size_t)cy * W + cx;
          const float4 col = p.in[g], pos = p.posT[g], nrm = p.nrmTri[g], alb = p.albedo[g];
          const float2 lv = p.lvIn[g];
          q.c = v3(col.x, col.y, col.z);
          q.valid = inside && __float_as_int(nrm.w) >= 0;
          q.P = v3(pos.x, pos.y, pos.z);
          q.l = lv.x;
          q.N = v3(nrm.x, nrm.y, nrm.z);
          q.v = lv.y;
          q.A = v3(alb.x, alb.y, alb.z);
        }
        float n = 1.0f;
        if (nl >= 0) {
          const float d = dot(Np, q.N);
          n = d > 0.0f ? d : 0.0f;
          for (int j = 0; j < nl; j++) n = n * n;
        }
        float a = 0.0f;
        if (zOn) a = a + fabsf(dot(Np, q.P - Pp)) / zden;
        if (lOn) a = a + fabsf(q.l - lvP.x) / lden;
        if (aOn) {
          const V3 D = q.A - Ap;
          a = a + dot(D, D) / p.albDen;
        }
        float w = (k * n) * ptm_expf(-a);
        w = q.valid ? w : 0.0f;
        const V3 cq = q.valid ? q.c : v3(0.0f, 0.0f, 0.0f);
        const float vq = q.valid ? q.v : 0.0f;
        sw = sw + w;
        sum = sum + cq * w;
        svar = svar + vq * (w * w);
      }
    }
    if (sw > 0.0f) {
      out = make_float4(sum.x / sw, sum.y / sw, sum.z / sw, cp.w);
      vOut = svar / (sw * sw);
    }
  }
  p.out[i] = out;
  // a miss pixel's colour is copied, so is its l
  if (p.lvOut) p.lvOut[i] = make_float2(hitP ? lumTm(out, p.limit) : lvP.x, vOut);
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
  const dim3 grid((p.width + ATROUS_TILE - 1) / ATROUS_TILE, (p.height + ATROUS_TILE - 1) / ATROUS_TILE);
  const dim3 block(ATROUS_TILE * ATROUS_TILE);
  if (p.stride <= ATROUS_LDS_STRIDE) {
    const int R = ATROUS_TILE + 4 * p.stride;
    const size_t lds = (size_t)4 * R * R * sizeof(float4);
    hipLaunchKernelGGL((atrousVarKernel<true>), grid, block, lds, s, p);
  } else {
    hipLaunchKernelGGL((atrousVarKernel<false>), grid, block, 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace pt
