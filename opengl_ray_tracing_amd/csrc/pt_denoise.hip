// pt_denoise.hip -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of the running
// mean, steered by the guide buffers (pt_abi.h pt_denoise). One launch per pass; a block filters a
// 16 x 16 tile, one lane per pixel. tests/denoise_ref.py is the specification: every f32 operation
// below is one of its operations, in its order, so the output equals it bit for bit (no fused
// multiply-adds, IEEE division, ptm_expf shared with the host).
//
// Per pixel a pass reads 5 float4 (colour, tone-mapped colour, position + t, normal + triangle,
// albedo) of 25 taps. tm(c) is computed once per pixel per pass: each pass writes tm(out) beside
// out as a fourth plane for the next pass (atrousTmKernel writes the first pass's from the
// accumulation), so a tap never recomputes it.
//  * stride <= ATROUS_LDS_STRIDE: the tile and its 2 x stride halo are staged in LDS as four
//    float4 per pixel -- (c.rgb, valid), (tm.rgb, A.r), (P.xyz, A.g), (N.xyz, A.b) -- 25.6 KB at
//    stride 1, 36.9 KB at stride 2; the taps are ds_read_b128. Staging copies bits: no operation
//    changes.
//  * larger strides: a tile's halo would be 3 x the tile and more, so the taps are direct 16-byte
//    loads (the planes sit in the Infinity Cache).
// Everything that depends only on the centre is hoisted; the tap loop has no divergent branch:
// a tap outside the image or on a miss pixel gets w = 0 and colour 0 by select (the restatement
// does the same: adding +0 is exact).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

__global__ void atrousTmKernel(const float4* in, float4* tm, int n, float limit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 t = tonemapPixel(in[i], limit, 0.0f);
  tm[i] = make_float4(t.x, t.y, t.z, 0.0f);
}

// one tap's data
struct TapPx {
  V3 c, tm, P, N, A;
  bool valid;
};

template <bool STAGE>
__global__ __launch_bounds__(ATROUS_TILE* ATROUS_TILE) void atrousKernel(AtrousParams p) {
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
        const float4 col = p.in[g], tm = p.tmIn[g], pos = p.posT[g], nrm = p.nrmTri[g], alb = p.albedo[g];
        a = make_float4(col.x, col.y, col.z, __int_as_float(__float_as_int(nrm.w) >= 0 ? 1 : 0));
        b = make_float4(tm.x, tm.y, tm.z, alb.x);
        c = make_float4(pos.x, pos.y, pos.z, alb.y);
        d = make_float4(nrm.x, nrm.y, nrm.z, alb.z);
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
  float4 out = cp;
  if (__float_as_int(nrmP.w) >= 0) {
    const float4 tmP4 = p.tmIn[i], posP = p.posT[i], albP = p.albedo[i];
    const V3 Tp = v3(tmP4.x, tmP4.y, tmP4.z), Pp = v3(posP.x, posP.y, posP.z), Np = v3(nrmP.x, nrmP.y, nrmP.z),
             Ap = v3(albP.x, albP.y, albP.z);
    const float zden = p.sigmaZ * posP.w;
    const bool zOn = p.sigmaZ > 0.0f, cOn = p.colOn != 0, aOn = p.albOn != 0;
    const int nl = p.normalLog2;
    float sw = 0.0f;
    V3 sum = v3(0.0f, 0.0f, 0.0f);
    for (int dy = -2; dy <= 2; dy++) {
      const int ady = dy < 0 ? -dy : dy;
      const float hy = ady == 0 ? 0.375f : (ady == 1 ? 0.25f : 0.0625f);
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const int adx = dx < 0 ? -dx : dx;
        const float hx = adx == 0 ? 0.375f : (adx == 1 ? 0.25f : 0.0625f);
        const float k = hx * hy;  // exact in f32
        TapPx q;
        if (STAGE) {
          const int li = (ly + 2 * s + s * dy) * R + (lx + 2 * s + s * dx);
          const float4 a = s_px[li], b = s_px[R * R + li], c = s_px[2 * R * R + li], d = s_px[3 * R * R + li];
          q.c = v3(a.x, a.y, a.z);
          q.valid = __float_as_int(a.w) != 0;
          q.tm = v3(b.x, b.y, b.z);
          q.P = v3(c.x, c.y, c.z);
          q.N = v3(d.x, d.y, d.z);
          q.A = v3(b.w, c.w, d.w);
        } else {
          const int qx = px + s * dx, qy = py + s * dy;
          const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
          const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);  // the load stays in the image
          const size_t g = (size_t)cy * W + cx;
          const float4 col = p.in[g], tm = p.tmIn[g], pos = p.posT[g], nrm = p.nrmTri[g], alb = p.albedo[g];
          q.c = v3(col.x, col.y, col.z);
          q.valid = inside && __float_as_int(nrm.w) >= 0;
          q.tm = v3(tm.x, tm.y, tm.z);
          q.P = v3(pos.x, pos.y, pos.z);
          q.N = v3(nrm.x, nrm.y, nrm.z);
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
        if (cOn) {
          const V3 D = q.tm - Tp;
          a = a + dot(D, D) / p.colDen;
        }
        if (aOn) {
          const V3 D = q.A - Ap;
          a = a + dot(D, D) / p.albDen;
        }
        float w = (k * n) * ptm_expf(-a);
        w = q.valid ? w : 0.0f;
        const V3 cq = q.valid ? q.c : v3(0.0f, 0.0f, 0.0f);
        sw = sw + w;
        sum = sum + cq * w;
      }
    }
    if (sw > 0.0f) out = make_float4(sum.x / sw, sum.y / sw, sum.z / sw, cp.w);
  }
  p.out[i] = out;
  if (p.tmOut) {
    const V3 t = tonemapPixel(out, p.limit, 0.0f);
    p.tmOut[i] = make_float4(t.x, t.y, t.z, 0.0f);
  }
}

hipError_t launchAtrousTm(const float4* in, float4* tm, int n, float limit, hipStream_t s) {
  hipLaunchKernelGGL(atrousTmKernel, dim3((n + 255) / 256), dim3(256), 0, s, in, tm, n, limit);
  return hipGetLastError();
}

hipError_t launchAtrous(const AtrousParams& p, hipStream_t s) {
  const dim3 grid((p.width + ATROUS_TILE - 1) / ATROUS_TILE, (p.height + ATROUS_TILE - 1) / ATROUS_TILE);
  const dim3 block(ATROUS_TILE * ATROUS_TILE);
  if (p.stride <= ATROUS_LDS_STRIDE) {
    const int R = ATROUS_TILE + 4 * p.stride;
    const size_t lds = (size_t)4 * R * R * sizeof(float4);
    hipLaunchKernelGGL((atrousKernel<true>), grid, block, lds, s, p);
  } else {
    hipLaunchKernelGGL((atrousKernel<false>), grid, block, 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace pt
