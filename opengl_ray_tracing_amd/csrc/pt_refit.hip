// pt_refit.hip -- new vertex positions in place (pt_abi.h pt_update_geometry): the device path from the
// caller's vertex records to every buffer pt_upload_scene derives from the positions, without the host.
//
//   recordsKernel   one thread per triangle: the geometry record (the unit normal and plane offset in
//                   pt_scene_prep.cpp nrm3's operation order: this file is built like every device file,
//                   without FMA contraction and with IEEE division and sqrt), the pair record of
//                   triangles i and i + 1, the three shading normals of the hit record (its material id
//                   stays)
//   leafKernel      one thread per reachable leaf of the uploaded tree: the exact bounds of its (at most
//                   32) triangles, in index order, into refBox
//   levelKernel     one launch per height while a height holds more nodes than the tail's block: an
//                   internal node's box from its children's, left before right. The kernel boundary is
//                   the hand-off between heights.
//   tailKernel      one block for all remaining heights, __syncthreads() between them: the nodes of a
//                   height are written and read by threads of this one workgroup only, so the barrier
//                   (with its workgroup-scope fence) is the whole hand-off. No kernel here waits on
//                   another workgroup. The reference's SAH trees are chains (c2: depth 59, c4: 97) whose
//                   upper heights hold one or two nodes each: one launch instead of one per height.
//   wideKernel      one thread per device wide node of the uploaded tree: the three box float4 from its
//                   children's refBox (absent children stay +-inf; the references in the fourth stay)
//   leafBoxKernel   one thread per triangle: leafBox from refBox of the leaf whose id lo.w holds
//
// min / max are the reference's select forms (scene.cpp gmin / gmax), so a refitted box equals, bit for
// bit, the box the reference's builders store for the same triangles (tests/refit_ref.py restates it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_kernels.h"

namespace pt {

namespace {

constexpr int BT = 256;

__device__ __forceinline__ float gmin(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float gmax(float a, float b) { return (a < b) ? b : a; }

struct Geo {
  float4 p1, p2, p3, n;  // SceneView::geo
};

// pt_scene_prep.cpp prepareScene / nrm3
__device__ __forceinline__ Geo geoOf(const float* t) {
  const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
  const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
  const float cx = e1y * e2z - e2y * e1z;
  const float cy = e1z * e2x - e2z * e1x;
  const float cz = e1x * e2y - e2x * e1y;
  const float inv = 1.0f / sqrtf((cx * cx + cy * cy) + cz * cz);
  const float nx = cx * inv, ny = cy * inv, nz = cz * inv;
  const float w = (nx * t[0] + ny * t[1]) + nz * t[2];
  Geo g;
  g.p1 = make_float4(t[0], t[1], t[2], w);
  g.p2 = make_float4(t[3], t[4], t[5], 0.0f);
  g.p3 = make_float4(t[6], t[7], t[8], 0.0f);
  g.n = make_float4(nx, ny, nz, 0.0f);
  return g;
}

__global__ void __launch_bounds__(BT) recordsKernel(RefitParams p) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= p.nTri) return;
  float t[18];
  const float* v = p.verts + (size_t)i * p.stride;
  for (int k = 0; k < 18; k++) t[k] = v[k];
  const Geo A = geoOf(t);
  float4* g = p.geo + 4 * (size_t)i;
  g[0] = A.p1; g[1] = A.p2; g[2] = A.p3; g[3] = A.n;
  float4* h = p.hitRec + (size_t)i * HIT_F4;
  const float fid = h[2].y;
  h[0] = make_float4(t[9], t[10], t[11], t[12]);
  h[1] = make_float4(t[13], t[14], t[15], t[16]);
  h[2] = make_float4(t[17], fid, 0.0f, 0.0f);
  // pt_scene_prep.cpp buildPairs: triangle i + 1's record computed here again (zeros past the last)
  Geo B;
  B.p1 = B.p2 = B.p3 = B.n = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const bool more = i + 1 < p.nTri;
  if (more) {
    float u[9];
    for (int k = 0; k < 9; k++) u[k] = v[p.stride + k];
    B = geoOf(u);
  }
  float4* r = p.pairs + (size_t)i * PAIR_F4;
  r[0] = make_float4(A.p1.x, B.p1.x, A.p1.y, B.p1.y);
  r[1] = make_float4(A.p1.z, B.p1.z, A.p2.x, B.p2.x);
  r[2] = make_float4(A.p2.y, B.p2.y, A.p2.z, B.p2.z);
  r[3] = make_float4(A.p3.x, B.p3.x, A.p3.y, B.p3.y);
  r[4] = make_float4(A.p3.z, B.p3.z, A.n.x, B.n.x);
  r[5] = make_float4(A.n.y, B.n.y, A.n.z, B.n.z);
  r[6] = make_float4(A.p1.w, B.p1.w, __int_as_float(i), __int_as_float(more ? i + 1 : -1));
}

__global__ void __launch_bounds__(BT) leafKernel(const int2* topo, const int* byHeight, int nLeaves, const float4* geo,
                                                 float4* refBox) {
  const int j = blockIdx.x * BT + threadIdx.x;
  if (j >= nLeaves) return;
  const int k = byHeight[j];
  const int2 tp = topo[k];
  if (tp.y >= 0) return;  // an internal node without children: its box stays
  const int first = tp.x, count = -tp.y;
  float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
  for (int i = 0; i < count; i++) {
    const float4* g = geo + 4 * (size_t)(first + i);
    const float4 a = g[0], b = g[1], c = g[2];
    const float l[3] = {gmin(a.x, gmin(b.x, c.x)), gmin(a.y, gmin(b.y, c.y)), gmin(a.z, gmin(b.z, c.z))};
    const float h[3] = {gmax(a.x, gmax(b.x, c.x)), gmax(a.y, gmax(b.y, c.y)), gmax(a.z, gmax(b.z, c.z))};
    for (int x = 0; x < 3; x++) {
      lo[x] = i ? gmin(lo[x], l[x]) : l[x];
      hi[x] = i ? gmax(hi[x], h[x]) : h[x];
    }
  }
  refBox[2 * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
  refBox[2 * (size_t)k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

// an internal node's box from its children's; a node without a child keeps its box
__device__ __forceinline__ void refitNode(const int2* topo, int k, float4* refBox) {
  const int2 tp = topo[k];
  float4 lo, hi;
  if (tp.x > 0) {
    lo = refBox[2 * (size_t)tp.x];
    hi = refBox[2 * (size_t)tp.x + 1];
    if (tp.y > 0) {
      const float4 rl = refBox[2 * (size_t)tp.y], rh = refBox[2 * (size_t)tp.y + 1];
      lo = make_float4(gmin(lo.x, rl.x), gmin(lo.y, rl.y), gmin(lo.z, rl.z), 0.0f);
      hi = make_float4(gmax(hi.x, rh.x), gmax(hi.y, rh.y), gmax(hi.z, rh.z), 0.0f);
    }
  } else if (tp.y > 0) {
    lo = refBox[2 * (size_t)tp.y];
    hi = refBox[2 * (size_t)tp.y + 1];
  } else {
    return;
  }
  refBox[2 * (size_t)k] = make_float4(lo.x, lo.y, lo.z, 0.0f);
  refBox[2 * (size_t)k + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

__global__ void __launch_bounds__(BT) levelKernel(const int2* topo, const int* byHeight, int begin, int end,
                                                  float4* refBox) {
  const int j = begin + blockIdx.x * BT + threadIdx.x;
  if (j < end) refitNode(topo, byHeight[j], refBox);
}

// one block: heights h0 .. h1 - 1 in order, each after the barrier behind the one below it
__global__ void __launch_bounds__(REFIT_TAIL) tailKernel(const int2* topo, const int* byHeight, const int* heightStart,
                                                         int h0, int h1, float4* refBox) {
  for (int h = h0; h < h1; h++) {
    const int begin = heightStart[h], end = heightStart[h + 1];
    for (int j = begin + (int)threadIdx.x; j < end; j += REFIT_TAIL) refitNode(topo, byHeight[j], refBox);
    __syncthreads();
  }
}

// pt_scene_prep.cpp encodeWideTree's box layout, its boxes not widened (the uploaded tree's are exact)
__global__ void __launch_bounds__(BT) wideKernel(const int2* devKids, int nDev, const float4* refBox, float4* bvh) {
  const int id = blockIdx.x * BT + threadIdx.x;
  if (id >= nDev) return;
  const int2 kid = devKids[id];
  const float inf = INFINITY;
  float4 la = make_float4(inf, inf, inf, 0.0f), lb = make_float4(-inf, -inf, -inf, 0.0f);
  float4 ra = la, rb = lb;
  if (kid.x > 0) { la = refBox[2 * (size_t)kid.x]; lb = refBox[2 * (size_t)kid.x + 1]; }
  if (kid.y > 0) { ra = refBox[2 * (size_t)kid.y]; rb = refBox[2 * (size_t)kid.y + 1]; }
  float4* r = bvh + 4 * (size_t)id;
  r[0] = make_float4(la.x, ra.x, la.y, ra.y);
  r[1] = make_float4(la.z, ra.z, lb.x, rb.x);
  r[2] = make_float4(lb.y, rb.y, lb.z, rb.z);
}

__global__ void __launch_bounds__(BT) leafBoxKernel(int nTri, const float4* refBox, float4* leafBox) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= nTri) return;
  const float idBits = leafBox[2 * (size_t)i].w;
  const int k = __float_as_int(idBits);
  if (k < 0) return;  // in no reference leaf: the empty box stays
  const float4 lo = refBox[2 * (size_t)k], hi = refBox[2 * (size_t)k + 1];
  leafBox[2 * (size_t)i] = make_float4(lo.x, lo.y, lo.z, idBits);
  leafBox[2 * (size_t)i + 1] = make_float4(hi.x, hi.y, hi.z, 0.0f);
}

inline int blocks(long n) { return (int)((n + BT - 1) / BT); }

}  // namespace

hipError_t launchRefit(const RefitParams& p, const RefitTables& t, const int* hostStart, hipEvent_t* ev, hipStream_t s) {
  if (!t.ready || p.nTri < 1 || p.stride < 18) return hipErrorInvalidValue;
  auto mark = [&](int k) { return ev ? hipEventRecord(ev[k], s) : hipSuccess; };
  hipError_t e = mark(0);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(recordsKernel, dim3(blocks(p.nTri)), dim3(BT), 0, s, p);
  if ((e = mark(1)) != hipSuccess) return e;
  const int nLeaves = hostStart[1];
  if (nLeaves > 0)
    hipLaunchKernelGGL(leafKernel, dim3(blocks(nLeaves)), dim3(BT), 0, s, t.topo, t.byHeight, nLeaves, p.geo, p.refBox);
  for (int h = 1; h < t.tailFrom; h++)
    hipLaunchKernelGGL(levelKernel, dim3(blocks(hostStart[h + 1] - hostStart[h])), dim3(BT), 0, s, t.topo, t.byHeight,
                       hostStart[h], hostStart[h + 1], p.refBox);
  if (t.tailFrom < t.heights)
    hipLaunchKernelGGL(tailKernel, dim3(1), dim3(REFIT_TAIL), 0, s, t.topo, t.byHeight, t.heightStart, t.tailFrom,
                       t.heights, p.refBox);
  if ((e = mark(2)) != hipSuccess) return e;
  if (p.nDevNodes > 0)
    hipLaunchKernelGGL(wideKernel, dim3(blocks(p.nDevNodes)), dim3(BT), 0, s, t.devKids, p.nDevNodes, p.refBox, p.bvh);
  if (p.leafBox) hipLaunchKernelGGL(leafBoxKernel, dim3(blocks(p.nTri)), dim3(BT), 0, s, p.nTri, p.refBox, p.leafBox);
  if ((e = mark(3)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace pt
