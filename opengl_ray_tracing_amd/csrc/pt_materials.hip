// pt_materials.hip -- new materials in place (pt_abi.h pt_update_materials): the device path from the
// caller's material records (Triangle_encoded floats 18..35 per triangle) to the two things
// pt_upload_scene derives from them -- the table of distinct materials (SceneView::mats) and each
// triangle's id in its hit record -- without the host.
//
// The table is pt_scene_prep.cpp materialTable's: keys compared as 18 uint32, numbered by their first
// appearance in triangle order. The order therefore comes from a scan over "triangle i is the smallest
// index with its key", never from the order in which atomics land (pt_build.hip states the same rule for
// the builder): every run gives the same table, bit for bit a fresh upload's.
//
//   insertKernel   one thread per triangle: its 18 key words stay in registers while it probes an
//                  open-addressed table of triangle indices (a power of two >= 2 * nTri slots, -1 empty,
//                  linear probing). An empty slot is claimed by atomicCAS; a slot whose representative
//                  has this key takes atomicMin(slot, i); any other slot is passed. Every value a slot
//                  ever holds has its claimer's key, so comparing against whichever representative is
//                  read -- also a stale one -- is correct while other threads lower it, and all triangles
//                  of one key end in one slot: the first that claimed for that key lies before every
//                  empty slot of their common probe sequence, and slots are never emptied. The thread
//                  remembers its slot. Within a wave only the first lane of each run of equal keys
//                  probes; the lanes behind it, which cannot be a first appearance, take its slot.
//   firstKernel    flag[i] = (slot of i holds i): i is its key's first appearance
//   (hipcub)       exclusive scan of the flags: rank[i] = first appearances before i, the id of a first
//   scatterKernel  every triangle writes its id -- rank of its slot's triangle -- as int bits into
//                  hitRec[i][2].y and nothing else of the record (pt_refit.hip preserves that float: this
//                  is its mirror image); a first appearance writes its table entry; the last triangle
//                  writes the count
//
// The kernel boundaries are the hand-offs; no kernel waits on another workgroup.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "pt_kernels.h"

namespace pt {

namespace {

constexpr int BT = 256;  // four waves of 64: the probe loops diverge per lane, nothing is shared in a block

struct Key {
  uint32_t w[MAT_KEY];
};

__device__ __forceinline__ Key loadKey(const MaterialParams& p, int i) {
  // 4-byte alignment is all the caller owes: dword loads
  const uint32_t* r = reinterpret_cast<const uint32_t*>(p.mats) + (size_t)i * (size_t)p.stride;
  Key k;
#pragma unroll
  for (int j = 0; j < MAT_KEY; j++) k.w[j] = r[j];
  return k;
}

__device__ __forceinline__ uint32_t hashKey(const Key& k) {
  uint32_t h = 0x9e3779b9u;
#pragma unroll
  for (int j = 0; j < MAT_KEY; j++) {
    uint32_t x = k.w[j] * 0xcc9e2d51u;
    x = (x << 15) | (x >> 17);
    h ^= x * 0x1b873593u;
    h = ((h << 13) | (h >> 19)) * 5u + 0xe6546b64u;
  }
  h ^= h >> 16; h *= 0x85ebca6bu;
  h ^= h >> 13; h *= 0xc2b2ae35u;
  return h ^ (h >> 16);
}

__device__ __forceinline__ bool sameKey(const MaterialParams& p, const Key& k, int other) {
  const uint32_t* r = reinterpret_cast<const uint32_t*>(p.mats) + (size_t)other * (size_t)p.stride;
  for (int j = 0; j < MAT_KEY; j++)
    if (r[j] != k.w[j]) return false;
  return true;
}

__global__ void __launch_bounds__(BT) insertKernel(MaterialParams p, MaterialTables t) {
  const int i = blockIdx.x * BT + threadIdx.x;
  const bool valid = i < p.nTri;  // no early return: the wave's lanes exchange keys and slots below
  const int lane = (int)(threadIdx.x & 63u);
  Key k;
  if (valid) {
    k = loadKey(p, i);
  } else {
#pragma unroll
    for (int j = 0; j < MAT_KEY; j++) k.w[j] = 0u;
  }
  // Meshes share one material, so most triangles have their predecessor's key (pt_scene_prep.cpp
  // materialTable takes the same shortcut). Such a triangle is never a first appearance, and its slot is
  // its predecessor's: only the heads of the wave's runs of equal keys probe -- lane 0 always -- and the
  // other lanes take their head's slot. A million triangles of one material are then 16 K inserts,
  // not a million atomics on one word.
  bool same = lane > 0;
#pragma unroll
  for (int j = 0; j < MAT_KEY; j++) same &= (uint32_t)__shfl_up((int)k.w[j], 1) == k.w[j];
  const bool head = valid && !same;
  const uint32_t mask = (uint32_t)t.nSlots - 1u;
  uint32_t h = hashKey(k) & mask;
  if (head) {
    // at most nSlots steps: the table holds at least nTri empty slots, so a probe ends long before
    for (int step = 0; step < t.nSlots; step++, h = (h + 1u) & mask) {
      int rep = __hip_atomic_load(&t.slots[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (rep < 0) {
        rep = atomicCAS(&t.slots[h], -1, i);
        if (rep < 0) break;  // claimed
      }
      if (sameKey(p, k, rep)) {
        if (i < rep) atomicMin(&t.slots[h], i);
        break;
      }
    }
  }
  // every lane again: the slot of the nearest head at or below this lane (lane 0 of a wave with a valid
  // lane is a head, and the valid lanes are the wave's first)
  const unsigned long long heads = __ballot(head);
  const unsigned long long below = heads & (~0ull >> (63 - lane));
  const int from = below ? 63 - __clzll((long long)below) : lane;
  h = (uint32_t)__shfl((int)h, from);
  if (valid) t.slotOf[i] = (int)h;
}

__global__ void __launch_bounds__(BT) firstKernel(int nTri, MaterialTables t) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i < nTri) t.flag[i] = t.slots[t.slotOf[i]] == i ? 1 : 0;
}

__global__ void __launch_bounds__(BT) scatterKernel(MaterialParams p, MaterialTables t) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= p.nTri) return;
  const int rep = t.slots[t.slotOf[i]];
  const int id = t.rank[rep];
  p.hitRec[(size_t)i * HIT_F4 + 2].y = __int_as_float(id);
  if (i == p.nTri - 1) *t.count = t.rank[i] + t.flag[i];
  if (rep != i) return;
  // the entry as uploaded: Triangle_encoded floats 16..35, whose first two no kernel reads (zeros here)
  const Key k = loadKey(p, i);
  float f[4 * MAT_F4];
  f[0] = f[1] = 0.0f;
#pragma unroll
  for (int j = 0; j < MAT_KEY; j++) f[2 + j] = __uint_as_float(k.w[j]);
  float4* m = p.table + (size_t)id * MAT_F4;
#pragma unroll
  for (int j = 0; j < MAT_F4; j++) m[j] = make_float4(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3]);
}

inline int blocks(long n) { return (int)((n + BT - 1) / BT); }

}  // namespace

int materialSlots(int nTri) {
  int n = 2;
  while (n < 2 * nTri) n *= 2;
  return n;
}

hipError_t materialScanBytes(int nTri, size_t* bytes) {
  int* none = nullptr;
  return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, none, none, nTri, nullptr);
}

hipError_t launchMaterials(const MaterialParams& p, const MaterialTables& t, hipEvent_t* ev, hipStream_t s) {
  if (p.nTri < 1 || p.stride < MAT_KEY || t.nSlots < 2 * p.nTri || (t.nSlots & (t.nSlots - 1))) return hipErrorInvalidValue;
  auto mark = [&](int k) { return ev ? hipEventRecord(ev[k], s) : hipSuccess; };
  hipError_t e = mark(0);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(t.slots, 0xff, (size_t)t.nSlots * sizeof(int), s)) != hipSuccess) return e;
  hipLaunchKernelGGL(insertKernel, dim3(blocks(p.nTri)), dim3(BT), 0, s, p, t);
  if ((e = mark(1)) != hipSuccess) return e;
  hipLaunchKernelGGL(firstKernel, dim3(blocks(p.nTri)), dim3(BT), 0, s, p.nTri, t);
  size_t bytes = t.scanBytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t.scanTmp, bytes, t.flag, t.rank, p.nTri, s)) != hipSuccess) return e;
  if ((e = mark(2)) != hipSuccess) return e;
  hipLaunchKernelGGL(scatterKernel, dim3(blocks(p.nTri)), dim3(BT), 0, s, p, t);
  if ((e = mark(3)) != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace pt
