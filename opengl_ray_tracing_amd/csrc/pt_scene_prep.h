// pt_scene_prep.h -- the host-only half of a scene upload (pt_scene_prep.cpp): the caller's raw
// arrays checked and re-laid out for the device, and the tables a geometry update refits by. No HIP
// runtime call and no context: pt_scene_upload.cpp uploads what this prepares, and
// tests/native/scene_prep_check.cpp dumps it on a machine without a GPU. Internal: not installed.
#pragma once
#include <climits>
#include <string>
#include <vector>

#include "pt_kernels.h"

namespace pt {

// The caller's nodes (the reference encoding: 12 f32 per node -- left, right, -, count, index, -, box
// lo, box hi -- dummy node 0, root 1), read in one place. The array is outside input: an integer field
// that is a NaN or outside [-2^31, 2^31) reads as INT_MIN (what the plain cast gave on x86, where it is
// undefined behaviour), so it names no child, no leaf, or a leaf out of bounds; every other value is
// truncated as ivec3(texelFetch) does (pass1.fsh:238-243).
struct NodeView {
  const float* nodes;
  int nNodes;
  static int toInt(float v) { return v >= -2147483648.0f && v < 2147483648.0f ? (int)v : INT_MIN; }
  const float* at(int k) const { return nodes + (size_t)k * 12; }
  int left(int k) const { return toInt(at(k)[0]); }
  int right(int k) const { return toInt(at(k)[1]); }
  int child(int k, int c) const { return toInt(at(k)[c]); }
  int count(int k) const { return toInt(at(k)[3]); }  // > 0: a leaf
  int index(int k) const { return toInt(at(k)[4]); }  // a leaf's first triangle
  const float* lo(int k) const { return at(k) + 6; }
  const float* hi(int k) const { return at(k) + 9; }
  bool inRange(int k) const { return k > 0 && k < nNodes; }
};

// A tree in the reference node encoding re-laid out as device wide nodes (pt_kernels.h
// SceneView::bvh).
struct WideTree {
  std::vector<float4> bvh;
  std::vector<int> ids;  // device id -> node id
  int rootRef = REF_NONE, nDev = 0, depth = 0;
};

// Everything pt_upload_scene derives on the host from the caller's arrays,
// computed once and uploaded to every device of a context.
struct SceneHost {
  int nTri = 0, nNodes = 0;
  std::vector<float4> geo, pairs;
  std::vector<float4> hit, mats;  // SceneView::hitRec / mats
  WideTree ref;
  std::vector<int2> topo;         // the uploaded tree's topology (pt_kernels.h RefitTables::topo), reachable nodes
  std::vector<float4> refBox;     // every reference node's box (lo, hi)
  // the runtime's own tree and the reference facts its results are checked against
  bool fast = false;
  bool deviceBuild = false;  // the tree itself is built on each device (pt_build.hip) by uploadScene
  float accelMs = 0.0f;      // host build time (deviceBuild false)
  int accelNodes = 0;
  float sceneScale = 0.0f;   // host build: the scale its boxes' widening used (prepareAccel: the origin domain)
  std::vector<float> accelRef;  // host build: its nodes in the reference encoding (encodeWide4)
  WideTree fastTree;
  std::vector<float4> fpairs, leafBox;
  std::vector<int> order, leafOf, parent;
};

// host-side re-layout of the caller's arrays (pt_upload_scene); "" or the reason they are malformed
std::string prepareScene(const float* tris, int nTri, const float* nodes, int nNodes, SceneHost& h, bool hostBuild);

// The material table of n material records (record i: the 18 floats at mats + i * stride, Triangle_encoded
// floats 18..35): distinct keys, compared bit for bit as 18 uint32 (+0 and -0 differ, two NaNs of the same
// bits are one key), numbered by their first appearance in triangle order. ids: each triangle's id;
// first: per id the triangle it first appears at. Returns the number of distinct keys. prepareScene's
// table, and what pt_update_materials must reproduce on the device (pt_materials.hip).
int materialTable(const float* mats, int n, int stride, std::vector<int>& ids, std::vector<int>& first);

// The runtime tree (reference encoding, root 1) collapsed to 4-wide nodes (pt_trace.h traceRay4).
// Precondition: nodes is a builder's own tree (buildAccel's, or refNodes of the device builder's), never
// the caller's array: children in range, every count and index a whole number below 2^31 -- a count in
// (0, 1) would read as an internal node here.
void encodeWide4(const float* nodes, int nNodes, int nTri, float inflate, float inflateAbs, std::vector<float4>& out,
                 int& rootRef, int& nDev, int& depth);

// the device builder's nodes (pt_build.hip BuildNode) in the reference encoding
std::vector<float> refNodes(const std::vector<BuildNode>& bn, int leafSize);

// The host form of pt_kernels.h RefitTables, from the uploaded tree's topology (SceneHost::topo) and
// its device order (WideTree::ids): the reachable nodes sorted by height (a leaf 0, an internal node
// one more than its higher child), so that every height is refitted after the ones below it, and
// each device wide node's children.
struct RefitHost {
  std::vector<int> byHeight, heightStart;  // heightStart: heights + 1 offsets into byHeight
  std::vector<int2> devKids;
  int heights = 0, tailFrom = 0;
};
RefitHost refitTables(const std::vector<int2>& topo, const std::vector<int>& order);

}  // namespace pt
