// pt_scene_prep.cpp -- the host-only scene preparation of pt_upload_scene (pt_scene_prep.h): the
// caller's triangles and nodes checked and re-laid out for the MI355X, the runtime tree's host build,
// and the height tables of pt_update_geometry. Plain C++ over the HIP vector types: no HIP runtime
// call, no context.
//
// Compiled with -ffp-contract=off so the per-triangle unit normal and plane
// offset precomputed here round exactly like the reference computes them
// inline (pass1.fsh:263, :273).
#include "pt_scene_prep.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>

#include "pt_accel.h"

namespace pt {

static inline void nrm3(const float* a, const float* b, const float* c, float N[3]) {
  // normalize(cross(p2 - p1, p3 - p1)), glm order (oracle: hitTriangle)
  float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
  float e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
  float cx = e1y * e2z - e2y * e1z;
  float cy = e1z * e2x - e2z * e1x;
  float cz = e1x * e2y - e2x * e1y;
  float inv = 1.0f / std::sqrt((cx * cx + cy * cy) + cz * cz);
  N[0] = cx * inv; N[1] = cy * inv; N[2] = cz * inv;
}

// A tree in the reference node encoding (12 f32 per node, dummy node 0, root 1)
// re-laid out as device wide nodes (pt_kernels.h SceneView::bvh). inflate > 0
// widens every box outward by that relative amount plus inflateAbs (the
// runtime's own tree: conservative, so a ray that hits a triangle always enters
// its boxes).
static std::string encodeWideTree(const float* nodes, int nNodes, int nTri, float inflate, WideTree& out,
                                  float inflateAbs = 0.0f) {
  const NodeView nv{nodes, nNodes};
  auto isInternal = [&](int k) { return nv.inRange(k) && nv.count(k) <= 0; };
  // depth of the reachable tree (bounds the traversal stack; rejects cycles)
  int depth = 0;
  {
    std::vector<std::pair<int, int>> st{{1, 1}};
    long visits = 0;
    while (!st.empty()) {
      auto [k, d] = st.back();
      st.pop_back();
      if (++visits > 2L * nNodes) return "node graph is not a tree (cycle)";
      depth = std::max(depth, d);
      if (nv.count(k) > 0) continue;
      int L = nv.left(k), R = nv.right(k);
      if (nv.inRange(L)) st.push_back({L, d + 1});
      if (nv.inRange(R)) st.push_back({R, d + 1});
    }
  }
  // Device ids of the reachable internal nodes: the first LDS_NODES in
  // breadth-first order from the root (the top of the tree, which every ray
  // walks: the megakernel stages exactly these ids in LDS), the rest in the
  // tree's id order (the reference's preorder, which keeps subtrees together).
  // Only the storage order changes; traversal visits the same nodes in the same
  // order.
  std::vector<int> newId(nNodes, -1), order;
  {
    std::vector<char> reach(nNodes, 0);
    std::vector<int> bfs;
    if (isInternal(1)) { bfs.push_back(1); reach[1] = 1; }
    for (size_t h = 0; h < bfs.size(); h++) {
      const int k = bfs[h];
      for (int c = 0; c < 2; c++) {
        const int ch = nv.child(k, c);
        if (isInternal(ch) && !reach[ch]) { reach[ch] = 1; bfs.push_back(ch); }
      }
    }
    for (size_t h = 0; h < bfs.size() && h < (size_t)LDS_NODES; h++) order.push_back(bfs[h]);
    for (int k : order) newId[k] = -2;
    for (int k = 1; k < nNodes; k++)
      if (reach[k] && newId[k] == -1) order.push_back(k);
    for (size_t i = 0; i < order.size(); i++) newId[order[i]] = (int)i;
  }
  std::string bad;
  // node references (ivec3(texelFetch) truncation, pass1.fsh:238-243)
  auto encodeRef = [&](int k) -> int {
    if (!nv.inRange(k)) return REF_NONE;
    int n = nv.count(k);
    if (n > 0) {
      int index = nv.index(k);
      if (index < 0 || (long)index + n > nTri) { bad = "leaf range out of bounds at node " + std::to_string(k); return REF_NONE; }
      if (n > MAX_LEAF) { bad = "leaf larger than 32 triangles at node " + std::to_string(k); return REF_NONE; }
      return (int)~(((uint32_t)index << LEAF_CNT_BITS) | (uint32_t)(n - 1));
    }
    return newId[k];
  };
  auto widen = [&](float4& lo, float4& hi) {
    if (inflate <= 0.0f && inflateAbs <= 0.0f) return;
    const float e[3] = {inflate * (std::fabs(lo.x) + std::fabs(hi.x) + (hi.x - lo.x)) + inflateAbs + 1e-30f,
                        inflate * (std::fabs(lo.y) + std::fabs(hi.y) + (hi.y - lo.y)) + inflateAbs + 1e-30f,
                        inflate * (std::fabs(lo.z) + std::fabs(hi.z) + (hi.z - lo.z)) + inflateAbs + 1e-30f};
    lo.x -= e[0]; lo.y -= e[1]; lo.z -= e[2];
    hi.x += e[0]; hi.y += e[1]; hi.z += e[2];
  };
  std::vector<float4>& bvh = out.bvh;
  bvh.assign(std::max<size_t>(order.size(), 1) * 4, make_float4(0, 0, 0, 0));
  const float inf = INFINITY;
  for (size_t id = 0; id < order.size(); id++) {
    const int k = order[id];
    int L = nv.left(k), R = nv.right(k);
    int lr = encodeRef(L), rr = encodeRef(R);
    if (!bad.empty()) return bad;
    float4 la = make_float4(inf, inf, inf, 0), lb = make_float4(-inf, -inf, -inf, 0);
    float4 ra = la, rb = lb;
    if (lr != REF_NONE) {
      const float *a = nv.lo(L), *b = nv.hi(L);
      la = make_float4(a[0], a[1], a[2], 0); lb = make_float4(b[0], b[1], b[2], 0);
      widen(la, lb);
    }
    if (rr != REF_NONE) {
      const float *a = nv.lo(R), *b = nv.hi(R);
      ra = make_float4(a[0], a[1], a[2], 0); rb = make_float4(b[0], b[1], b[2], 0);
      widen(ra, rb);
    }
    // children paired per component (left, right) so one packed op serves both boxes
    float refs[2];
    std::memcpy(&refs[0], &lr, 4);
    std::memcpy(&refs[1], &rr, 4);
    bvh[4 * id + 0] = make_float4(la.x, ra.x, la.y, ra.y);
    bvh[4 * id + 1] = make_float4(la.z, ra.z, lb.x, rb.x);
    bvh[4 * id + 2] = make_float4(lb.y, rb.y, lb.z, rb.z);
    bvh[4 * id + 3] = make_float4(refs[0], refs[1], 0.0f, 0.0f);
  }
  out.rootRef = encodeRef(1);
  if (!bad.empty()) return bad;
  out.nDev = (int)order.size();
  out.depth = depth;
  out.ids = std::move(order);
  return "";
}

// The runtime tree (reference encoding, 12 f32 per node, root 1) collapsed to
// 4-wide nodes (pt_trace.h traceRay4): each wide node takes a binary node's two
// children and keeps replacing its internal child of largest surface area by
// that child's two children until it has four (or only leaves). Wide nodes get
// breadth-first ids (the first ones are the top the kernels stage in LDS); the
// children's boxes are widened like encodeWideTree's; leaves keep their
// references into the pair records. depth: wide levels (root = 1).
// (Its input is the host builder's own tree, whose fields are whole numbers: a count read
// through the decoder is positive exactly when the float is.)
void encodeWide4(const float* nodes, int nNodes, int nTri, float inflate, float inflateAbs,
                 std::vector<float4>& out, int& rootRef, int& nDev, int& depth) {
  const NodeView nv{nodes, nNodes};
  auto isLeaf = [&](int k) { return nv.count(k) > 0; };
  auto area = [&](int k) {
    const float *l = nv.lo(k), *h = nv.hi(k);
    const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
    return dx * dy + dx * dz + dy * dz;
  };
  auto leafRef = [&](int k) {
    return (int)~(((uint32_t)nv.index(k) << LEAF_CNT_BITS) | (uint32_t)(nv.count(k) - 1));
  };
  out.clear();
  nDev = 0;
  depth = 1;
  if (nNodes < 2 || isLeaf(1)) {
    rootRef = nNodes >= 2 ? leafRef(1) : REF_NONE;
    out.assign(W4_F4, make_float4(0, 0, 0, 0));
    return;
  }
  std::vector<int> queue{1}, level{1};  // binary ids of the wide nodes, breadth-first, and their levels
  std::vector<std::array<int, 4>> kids;
  for (size_t q = 0; q < queue.size(); q++) {
    const int b = queue[q];
    std::array<int, 4> k = {nv.left(b), nv.right(b), 0, 0};
    int n = 2;
    while (n < 4) {
      int pick = -1;
      double pa = -1.0;
      for (int i = 0; i < n; i++)
        if (!isLeaf(k[i]) && area(k[i]) > pa) { pa = area(k[i]); pick = i; }
      if (pick < 0) break;
      const int c = k[pick];
      k[pick] = nv.left(c);
      k[n++] = nv.right(c);
    }
    for (int i = n; i < 4; i++) k[i] = 0;
    for (int i = 0; i < n; i++)
      if (!isLeaf(k[i])) {
        queue.push_back(k[i]);
        level.push_back(level[q] + 1);
        depth = std::max(depth, level[q] + 1);
      }
    kids.push_back(k);
  }
  nDev = (int)queue.size();
  std::vector<int> wideId(nNodes, -1);
  for (int i = 0; i < nDev; i++) wideId[queue[i]] = i;
  out.assign((size_t)nDev * W4_F4, make_float4(0, 0, 0, 0));
  for (int w = 0; w < nDev; w++) {
    float lo[3][4], hi[3][4];
    int ref[4];
    for (int i = 0; i < 4; i++) {
      const int c = kids[w][i];
      if (c <= 0) {
        ref[i] = REF_NONE;
        for (int a = 0; a < 3; a++) { lo[a][i] = INFINITY; hi[a][i] = -INFINITY; }
        continue;
      }
      ref[i] = isLeaf(c) ? leafRef(c) : wideId[c];
      for (int a = 0; a < 3; a++) {
        const float l = nv.lo(c)[a], h = nv.hi(c)[a];
        const float e = inflate * (std::fabs(l) + std::fabs(h) + (h - l)) + inflateAbs + 1e-30f;
        lo[a][i] = l - e;
        hi[a][i] = h + e;
      }
    }
    float4* r = &out[(size_t)w * W4_F4];
    for (int a = 0; a < 3; a++) {
      r[a] = make_float4(lo[a][0], lo[a][1], lo[a][2], lo[a][3]);
      r[3 + a] = make_float4(hi[a][0], hi[a][1], hi[a][2], hi[a][3]);
    }
    float fr[4];
    std::memcpy(fr, ref, sizeof(fr));
    r[6] = make_float4(fr[0], fr[1], fr[2], fr[3]);
  }
  rootRef = 0;
  (void)nTri;
}

// the device builder's nodes (pt_build.hip BuildNode, breadth-first from 0) in the
// reference encoding (BVHNode_encoded, main.cpp:69-73): build node k is node k + 1
std::vector<float> refNodes(const std::vector<BuildNode>& bn, int leafSize) {
  const int M = (int)bn.size();
  std::vector<float> out((size_t)(M + 1) * 12, 0.0f);
  for (int k = 0; k < M; k++) {
    const BuildNode& b = bn[k];
    float* o = out.data() + 12 * (size_t)(k + 1);
    int start, count, left, right;
    std::memcpy(&start, &b.lo.w, 4);
    std::memcpy(&count, &b.hi.w, 4);
    std::memcpy(&left, &b.clo.w, 4);
    std::memcpy(&right, &b.chi.w, 4);
    const bool leaf = count <= leafSize;
    o[0] = leaf ? 0.0f : (float)(left + 1);
    o[1] = leaf ? 0.0f : (float)(right + 1);
    o[3] = leaf ? (float)count : 0.0f;
    o[4] = leaf ? (float)start : 0.0f;
    o[6] = b.lo.x; o[7] = b.lo.y; o[8] = b.lo.z;
    o[9] = b.hi.x; o[10] = b.hi.y; o[11] = b.hi.z;
  }
  return out;
}

// pair records: position i holds triangles order[i] (x) and order[i + 1] (y,
// zeros past the last), PAIR_F4 float4 each (pt_trace.h pairTest), and the two triangles'
// uploaded indices as int bits in the last two floats (-1 past the last): a walk of the
// runtime's tree reads its winner's index with the winner's record (pairTestIds)
static void buildPairs(const std::vector<float4>& geo, const int* order, int nTri, std::vector<float4>& pairs) {
  pairs.assign((size_t)nTri * PAIR_F4, make_float4(0, 0, 0, 0));
  const float4 zero[4] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0),
                          make_float4(0, 0, 0, 0)};
  for (int i = 0; i < nTri; i++) {
    const float4* A = &geo[4 * (size_t)(order ? order[i] : i)];
    const float4* B = i + 1 < nTri ? &geo[4 * (size_t)(order ? order[i + 1] : i + 1)] : zero;
    float4* r = &pairs[(size_t)i * PAIR_F4];
    r[0] = make_float4(A[0].x, B[0].x, A[0].y, B[0].y);  // p1.x, p1.y
    r[1] = make_float4(A[0].z, B[0].z, A[1].x, B[1].x);  // p1.z, p2.x
    r[2] = make_float4(A[1].y, B[1].y, A[1].z, B[1].z);  // p2.y, p2.z
    r[3] = make_float4(A[2].x, B[2].x, A[2].y, B[2].y);  // p3.x, p3.y
    r[4] = make_float4(A[2].z, B[2].z, A[3].x, B[3].x);  // p3.z, Ng.x
    r[5] = make_float4(A[3].y, B[3].y, A[3].z, B[3].z);  // Ng.y, Ng.z
    const int ia = order ? order[i] : i, ib = i + 1 < nTri ? (order ? order[i + 1] : i + 1) : -1;
    float fa, fb;
    std::memcpy(&fa, &ia, sizeof(fa));
    std::memcpy(&fb, &ib, sizeof(fb));
    r[6] = make_float4(A[0].w, B[0].w, fa, fb);          // w = dot(Ng, p1); the uploaded indices
  }
}

// The runtime's own tree (a binned-SAH build over the uploaded triangles) and
// the reference facts a result found through it is checked against
// (pt_trace.h refReachable): each triangle's reference leaf and its box, every
// reference node's parent and box. Any triangle in two reference leaves, or a
// failed build, leaves the runtime on the reference tree alone (h.fast false).
static void prepareAccel(const float* tris, int nTri, const float* nodes, int nNodes, SceneHost& h, bool hostBuild) {
  h.fast = false;
  const NodeView nv{nodes, nNodes};
  std::vector<int>& leafOf = h.leafOf;
  std::vector<int>& parent = h.parent;
  leafOf.assign(nTri, -1);
  parent.assign(nNodes, 0);
  {
    std::vector<int> st{1};
    while (!st.empty()) {
      const int k = st.back();
      st.pop_back();
      if (nv.count(k) > 0) {
        const int index = nv.index(k);
        for (int i = index; i < index + nv.count(k); i++) {
          if (leafOf[i] != -1) return;  // a triangle in two leaves: reference tree only
          leafOf[i] = k;
        }
        continue;
      }
      for (int c = 0; c < 2; c++) {
        const int ch = nv.child(k, c);
        if (nv.inRange(ch)) {
          // refReachable's margin test needs every box inside its parent's (true
          // of the reference builders, which bound each node's own triangles)
          const float* pb = nv.at(k);
          const float* cb = nv.at(ch);
          for (int a = 0; a < 3; a++)
            if (!(pb[6 + a] <= cb[6 + a] && cb[9 + a] <= pb[9 + a])) return;
          parent[ch] = k;
          st.push_back(ch);
        }
      }
    }
  }
  h.leafBox.assign((size_t)nTri * 2, make_float4(0, 0, 0, 0));
  const float inf = INFINITY;
  for (int i = 0; i < nTri; i++) {
    // lo.w holds the reference leaf's node id (int bits), so the reachability check reads one
    // 32-byte record per hit instead of that record and a separate leaf-id array
    if (leafOf[i] < 0) {  // in no reference leaf: never a reference hit (empty box fails the margin test)
      h.leafBox[2 * (size_t)i] = make_float4(inf, inf, inf, 0.0f);
      h.leafBox[2 * (size_t)i + 1] = make_float4(-inf, -inf, -inf, 0.0f);
    } else {
      h.leafBox[2 * (size_t)i] = h.refBox[2 * (size_t)leafOf[i]];
      h.leafBox[2 * (size_t)i + 1] = h.refBox[2 * (size_t)leafOf[i] + 1];
    }
    int id = leafOf[i];
    std::memcpy(&h.leafBox[2 * (size_t)i].w, &id, sizeof(int));
  }
  // the tree itself: on the GPU by uploadScene (pt_build.hip), or here (scene.cpp's threaded binned SAH)
  if (!hostBuild) {
    h.deviceBuild = true;
    h.fast = true;
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<float> an;
  if (pt::buildAccel(tris, nTri, PT_ACCEL_LEAF, an, h.order) < 0 || an.size() / 12 >= (1u << 24)) return;
  h.accelNodes = (int)(an.size() / 12) - 1;
  h.accelRef = an;

  // Widened by 1e-5 of each box's own magnitude plus 3e-5 of the scene's, so that a ray that hits a
  // triangle enters every box around it although the walks' slab tests are fused (pt_trace.h visitNodeF,
  // traceRay4). THE ORIGIN DOMAIN -- the one derivation; pt_abi.h, DESIGN.md and pt_trace.h quote it.
  // s = sceneScale, the largest coordinate magnitude of the scene (of the tree's root box: the device
  // builder's encodeKernel takes it from there). One fused slab value of plane p, origin o, direction d on
  // one axis is fl(fma(p, inv, noi)) with inv = fl(1/d) and noi = fl(-o inv): three roundings e1, e2, e3,
  // each at most 2^-24 relative. Times d, in position space, it differs from the exact p - o by
  //   (p - o) e1 + o e2 + (p - o) e3  <=  (2 |p - o| + |o|) 2^-24.
  // With |o| <= K s and |p| <= s that is at most (3 K + 2) s 2^-24. An axis's two slab values move by that
  // much; its box planes were moved outwards by at least 3e-5 s, so while the first stays below the second
  // the computed slab of every axis still holds the exact ray's hit parameter, and the box passes.
  // 4 (3 K + 2) 2^-24 <= 3e-5 -- a factor 4 between rounding and widening -- holds for K <= 41.3: K = 32,
  // the largest power of two (K = 32: 5.8e-6 s against 3e-5 s, a factor 5.1; K = 64 would leave 2.6).
  // That is pt_kernels.h PT_ORIGIN_K. A ray is in domain iff max(|o.x|, |o.y|, |o.z|) <= 32 s
  // (originInDomain); any other ray, a NaN or infinite origin included, never enters this tree: the
  // query kernels send it through the reference-order walk of the uploaded tree per ray, a frame or
  // guide launch whose eye is outside runs without the runtime tree (pt_plan.h eyeInDomain).
  // tests/test_accel_domain.py restates the fused test on this tree's dumped boxes: no hit is lost out
  // to 16 K (the margin it pins), some are at 1e5 s and beyond.
  float sceneScale = 0.0f;
  for (int i = 0; i < nTri; i++)
    for (int k = 0; k < 9; k++) sceneScale = std::max(sceneScale, std::fabs(tris[(size_t)i * 36 + k]));
  h.sceneScale = sceneScale;
  if (!encodeWideTree(an.data(), (int)(an.size() / 12), nTri, 1e-5f, h.fastTree, 3e-5f * sceneScale).empty()) return;
  buildPairs(h.geo, h.order.data(), nTri, h.fpairs);
  h.accelMs = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  h.fast = true;
}

// The material table's numbering (pt_scene_prep.h): record i is the 18 floats at mats + i * stride,
// compared as 18 uint32, never as floats
int materialTable(const float* mats, int n, int stride, std::vector<int>& ids, std::vector<int>& first) {
  ids.assign(std::max(n, 0), 0);
  first.clear();
  std::map<std::array<uint32_t, 18>, int> seen;
  std::array<uint32_t, 18> lastKey{};
  int lastId = 0;
  for (int i = 0; i < n; i++) {
    std::array<uint32_t, 18> key;
    std::memcpy(key.data(), mats + (size_t)i * stride, sizeof(key));
    int id;
    if (i > 0 && key == lastKey) {  // meshes share one material: most lookups are this one
      id = lastId;
    } else if (auto it = seen.find(key); it == seen.end()) {
      id = (int)seen.size();
      seen.emplace(key, id);
      first.push_back(i);
    } else {
      id = it->second;
    }
    lastKey = key;
    lastId = id;
    ids[i] = id;
  }
  return (int)first.size();
}

// host-side re-layout of the caller's arrays (pt_upload_scene); "" or the reason they are malformed
std::string prepareScene(const float* tris, int nTri, const float* nodes, int nNodes, SceneHost& h, bool hostBuild) {
  h.nTri = nTri;
  h.nNodes = nNodes;
  // geometry records (+1 zero record past the last triangle)
  h.geo.assign((size_t)(nTri + 1) * 4, make_float4(0, 0, 0, 0));
  for (int i = 0; i < nTri; i++) {
    const float* t = tris + (size_t)i * 36;
    float N[3];
    nrm3(t, t + 3, t + 6, N);
    float w = (N[0] * t[0] + N[1] * t[1]) + N[2] * t[2];
    h.geo[4 * i + 0] = make_float4(t[0], t[1], t[2], w);
    h.geo[4 * i + 1] = make_float4(t[3], t[4], t[5], 0.0f);
    h.geo[4 * i + 2] = make_float4(t[6], t[7], t[8], 0.0f);
    h.geo[4 * i + 3] = make_float4(N[0], N[1], N[2], 0.0f);
  }
  // shading records: the normals and a material id per triangle; each distinct
  // material (Triangle_encoded floats 18..35, compared bit for bit) stored once
  h.hit.assign((size_t)nTri * HIT_F4, make_float4(0, 0, 0, 0));
  {
    std::vector<int> ids, first;
    materialTable(tris + 18, nTri, 36, ids, first);
    for (int i : first) {
      const float* t = tris + (size_t)i * 36;
      for (int k = 0; k < MAT_F4; k++) h.mats.push_back(make_float4(t[16 + 4 * k], t[17 + 4 * k], t[18 + 4 * k], t[19 + 4 * k]));
    }
    for (int i = 0; i < nTri; i++) {
      const float* t = tris + (size_t)i * 36;
      float fid;
      std::memcpy(&fid, &ids[i], 4);
      float4* r = &h.hit[(size_t)i * HIT_F4];
      r[0] = make_float4(t[9], t[10], t[11], t[12]);
      r[1] = make_float4(t[13], t[14], t[15], t[16]);
      r[2] = make_float4(t[17], fid, 0.0f, 0.0f);
    }
  }
  std::string bad = encodeWideTree(nodes, nNodes, nTri, 0.0f, h.ref);
  if (!bad.empty()) return bad;
  buildPairs(h.geo, nullptr, nTri, h.pairs);
  // what pt_update_geometry refits: every node's box, and the reachable tree's topology (a tree:
  // encodeWideTree has rejected cycles)
  const NodeView nv{nodes, nNodes};
  h.refBox.assign((size_t)nNodes * 2, make_float4(0, 0, 0, 0));
  for (int k = 0; k < nNodes; k++) {
    const float *lo = nv.lo(k), *hi = nv.hi(k);
    h.refBox[2 * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    h.refBox[2 * (size_t)k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
  h.topo.assign(nNodes, make_int2(0, 0));
  {
    std::vector<int> st{1};
    std::vector<char> seen(nNodes, 0);
    while (!st.empty()) {
      const int k = st.back();
      st.pop_back();
      if (seen[k]) continue;
      seen[k] = 1;
      if (nv.count(k) > 0) {
        h.topo[k] = make_int2(nv.index(k), -nv.count(k));
        continue;
      }
      int ch[2] = {nv.left(k), nv.right(k)};
      for (int& x : ch) {
        if (!nv.inRange(x)) x = 0;
        if (x) st.push_back(x);
      }
      h.topo[k] = make_int2(ch[0], ch[1]);
    }
  }
  prepareAccel(tris, nTri, nodes, nNodes, h, hostBuild);
  return "";
}

RefitHost refitTables(const std::vector<int2>& topo, const std::vector<int>& order) {
  RefitHost r;
  const int nNodes = (int)topo.size();
  std::vector<int> height(nNodes, -1), st{1};
  int heights = 0;
  while (!st.empty()) {
    const int k = st.back();
    const int2 tp = topo[k];
    int below = -1;
    bool wait = false;
    if (tp.y >= 0)
      for (int c : {tp.x, tp.y}) {
        if (c <= 0) continue;
        if (height[c] < 0) { st.push_back(c); wait = true; }
        else below = std::max(below, height[c]);
      }
    if (wait) continue;
    height[k] = below + 1;
    heights = std::max(heights, height[k] + 1);
    st.pop_back();
  }
  std::vector<int>& start = r.heightStart;
  start.assign(heights + 1, 0);
  for (int k = 1; k < nNodes; k++)
    if (height[k] >= 0) start[height[k] + 1]++;
  for (int h = 0; h < heights; h++) start[h + 1] += start[h];
  std::vector<int> at(start.begin(), start.end() - 1);
  r.byHeight.resize(start[heights]);
  for (int k = 1; k < nNodes; k++)
    if (height[k] >= 0) r.byHeight[at[height[k]]++] = k;
  // launches while a height holds more nodes than the tail's block, then the tail
  int tailFrom = heights;
  while (tailFrom > 1 && start[tailFrom] - start[tailFrom - 1] <= REFIT_TAIL) tailFrom--;
  r.devKids.resize(order.size());
  for (size_t id = 0; id < r.devKids.size(); id++) r.devKids[id] = topo[order[id]];
  r.heights = heights;
  r.tailFrom = tailFrom;
  return r;
}

}  // namespace pt
