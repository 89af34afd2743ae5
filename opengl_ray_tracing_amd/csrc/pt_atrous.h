// pt_atrous.h -- the tile function of the two edge-avoiding a-trous filters (pt_denoise.hip,
// pt_variance.hip): everything their passes share, once. A block filters a 16 x 16 tile, one lane
// per pixel; a pass weighs the 25 taps of the 5 x 5 B3 kernel at its stride by the guides (normal,
// depth, albedo) and by one term of the filter's own, and writes the normalised sum.
//  * stride <= ATROUS_LDS_STRIDE: the tile and its 2 x stride halo are staged in LDS as four
//    float4 per pixel, 25.6 KB at stride 1, 36.9 KB at stride 2; the taps are ds_read_b128.
//    Staging copies bits: no operation changes. The first float4 is (c.rgb, valid); how the
//    guides and the term's own data share the other three is the term's (each filter keeps the
//    layout its taps were measured with).
//  * larger strides: a tile's halo would be 3 x the tile and more, so the taps are direct 16-byte
//    loads (the planes sit in the Infinity Cache), each address clamped into the image first.
// Everything that depends only on the centre is hoisted; the tap loop has no divergent branch:
// a tap outside the image or on a miss pixel gets w = 0 and colour 0 by select (the restatements
// do the same: adding +0 is exact). The order of the f32 operations is the restatements'
// (tests/denoise_ref.py, tests/variance_ref.py): in the exponent depth, the term's own, albedo.
//
// A Term supplies what differs between the filters: Params, the kernel's parameters (an
// AtrousCommon); Px and load(p, g), its own data of pixel g; pack / unpack, the staged layout of
// (P, N, A, Px); Term(p, i), what it reads of any centre, and centre<STAGE>(p, at, s_px), the rest
// of its set-up at a hit centre; range(p, e, a), its summand of the exponent a; accumulate(valid,
// e, w) and normalise(sw), its own sums beside sw and sum; write(p, out, hit), what it writes
// beside the colour for the next pass.
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

// where a lane is
struct AtrousAt {
  int W, H, s, R;      // the image, the stride, STAGE: the staged edge
  int px, py, lx, ly;  // its pixel, its place in the tile
};

template <class Term, bool STAGE>
__device__ __forceinline__ void atrousTile(const typename Term::Params& kernelArg, float4* s_px) {
  // s_px, STAGE: 4 planes of R x R pixels
  // a copy of its own: read through the reference to the kernel's argument, the direct kernels take 4 VGPRs more
  const typename Term::Params p = kernelArg;
  AtrousAt at;
  const int W = at.W = p.width, H = at.H = p.height, s = at.s = p.stride;
  const int lx = at.lx = threadIdx.x & (ATROUS_TILE - 1), ly = at.ly = threadIdx.x / ATROUS_TILE;
  const int x0 = blockIdx.x * ATROUS_TILE, y0 = blockIdx.y * ATROUS_TILE;
  const int px = at.px = x0 + lx, py = at.py = y0 + ly;
  const int R = at.R = ATROUS_TILE + 4 * s;
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
        a = make_float4(col.x, col.y, col.z, __int_as_float(__float_as_int(nrm.w) >= 0 ? 1 : 0));
        Term::pack(pos, nrm, alb, Term::load(p, g), b, c, d);
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
  Term term(p, i);
  float4 out = cp;
  const bool hitP = __float_as_int(nrmP.w) >= 0;
  if (hitP) {
    const float4 posP = p.posT[i], albP = p.albedo[i];
    const V3 Pp = v3(posP.x, posP.y, posP.z), Np = v3(nrmP.x, nrmP.y, nrmP.z), Ap = v3(albP.x, albP.y, albP.z);
    const float zden = p.sigmaZ * posP.w;
    const bool zOn = p.sigmaZ > 0.0f, aOn = p.albOn != 0;
    const int nl = p.normalLog2;
    term.template centre<STAGE>(p, at, s_px);
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
        // one tap's data
        V3 qc, qP, qN, qA;
        typename Term::Px qe;
        bool valid;
        if (STAGE) {
          const int li = (ly + 2 * s + s * dy) * R + (lx + 2 * s + s * dx);
          const float4 a = s_px[li], b = s_px[R * R + li], c = s_px[2 * R * R + li], d = s_px[3 * R * R + li];
          qc = v3(a.x, a.y, a.z);
          valid = __float_as_int(a.w) != 0;
          Term::unpack(b, c, d, qP, qN, qA, qe);
        } else {
          const int qx = px + s * dx, qy = py + s * dy;
          const bool inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
          const int cx = min(max(qx, 0), W - 1), cy = min(max(qy, 0), H - 1);  // the load stays in the image
          const size_t g = (size_t)cy * W + cx;
          const float4 col = p.in[g], pos = p.posT[g], nrm = p.nrmTri[g], alb = p.albedo[g];
          qc = v3(col.x, col.y, col.z);
          valid = inside && __float_as_int(nrm.w) >= 0;
          qP = v3(pos.x, pos.y, pos.z);
          qN = v3(nrm.x, nrm.y, nrm.z);
          qA = v3(alb.x, alb.y, alb.z);
          qe = Term::load(p, g);
        }
        float n = 1.0f;
        if (nl >= 0) {
          const float d = dot(Np, qN);
          n = d > 0.0f ? d : 0.0f;
          for (int j = 0; j < nl; j++) n = n * n;
        }
        float a = 0.0f;
        if (zOn) a = a + fabsf(dot(Np, qP - Pp)) / zden;
        term.range(p, qe, a);
        if (aOn) {
          const V3 D = qA - Ap;
          a = a + dot(D, D) / p.albDen;
        }
        float w = (k * n) * ptm_expf(-a);
        w = valid ? w : 0.0f;
        const V3 cq = valid ? qc : v3(0.0f, 0.0f, 0.0f);
        sw = sw + w;
        sum = sum + cq * w;
        term.accumulate(valid, qe, w);
      }
    }
    if (sw > 0.0f) {
      out = make_float4(sum.x / sw, sum.y / sw, sum.z / sw, cp.w);
      term.normalise(sw);
    }
  }
  p.out[i] = out;
  term.write(p, out, hitP);
}

// one pass: the staged kernel up to ATROUS_LDS_STRIDE, the direct one beyond
template <class Params>
static hipError_t launchAtrousPass(void (*staged)(Params), void (*direct)(Params), const Params& p, hipStream_t s) {
  const dim3 grid((p.width + ATROUS_TILE - 1) / ATROUS_TILE, (p.height + ATROUS_TILE - 1) / ATROUS_TILE);
  const dim3 block(ATROUS_TILE * ATROUS_TILE);
  if (p.stride <= ATROUS_LDS_STRIDE) {
    const int R = ATROUS_TILE + 4 * p.stride;
    const size_t lds = (size_t)4 * R * R * sizeof(float4);
    hipLaunchKernelGGL(staged, grid, block, lds, s, p);
  } else {
    hipLaunchKernelGGL(direct, grid, block, 0, s, p);
  }
  return hipGetLastError();
}

}  // namespace pt
