// pt_envupdate.hip -- the environment updated in place (pt_abi.h pt_update_env): the device steps
// pt_envcache.hip does not already have, between the caller's w*h*3 floats in device memory and the
// Env the frame kernels read. pt_env.cpp updateEnvOne strings them together with launchHdrCache,
// launchEnvPack, launchEnvCompact, launchEnvTrig and launchEnvLight.
//
//   envTexelsKernel   one thread per texel: its three floats -- through pt_rgbe.h pt_rgbe_quantise under
//                     PT_ENV_RGBE -- become the float4 texel; a caller's table entry (x, y, pdf) is split
//                     into the texel's w and the float2 table
//   the row form      pt_env.cpp envOne's host walk over the compact table (Env::cacheRow / cacheY), on
//                     the device, with the host loop's numbering:
//     rowCheckKernel  one block per row: every entry's x is the row's first; the row enters the
//                     first-row table of its x (atomicMin: the smallest row wins whatever the order)
//     rowIdKernel     one block: a row is a leader if it is the first of its x; leaders are numbered by
//                     a scan in row order -- the host loop's "by first appearance" -- and every row
//                     gets x | its leader's id << 16
//     rowYKernel      one block per row: a leader copies its y's to its id's row of cacheY, every other
//                     row compares its y's with its leader's
//   envDecodeKernel   the diagnostic behind pt_download_env forms 1 and 2
//
// The ids come from the scan, never from the order in which atomics land, so every run gives the same
// rows. Kernel boundaries are the hand-offs; no kernel waits on another workgroup. The flag words are
// zeroed by the caller's hipMemsetAsync on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_device.h"
#include "pt_envupdate.h"
#include "pt_kernels.h"
#include "pt_rgbe.h"

namespace pt {

namespace {

constexpr int BT = 256;
constexpr int SCAN_T = 1024;  // rowIdKernel's one block

__global__ void __launch_bounds__(BT) envTexelsKernel(const float* __restrict__ src3, const float* __restrict__ cache3,
                                                      int rgbe, float4* __restrict__ hdr, float2* __restrict__ samp,
                                                      float* __restrict__ quant3, int n) {
  const int k = blockIdx.x * BT + threadIdx.x;
  if (k >= n) return;
  const size_t k3 = 3 * (size_t)k;
  float r = src3[k3], g = src3[k3 + 1], b = src3[k3 + 2];
  if (rgbe) pt_rgbe_quantise(&r, &g, &b);
  float pdf = 0.0f;  // the library's table fills it (launchEnvPack)
  if (cache3) {
    samp[k] = make_float2(cache3[k3], cache3[k3 + 1]);
    pdf = cache3[k3 + 2];
  }
  hdr[k] = make_float4(r, g, b, pdf);
  if (quant3) {
    quant3[k3] = r;
    quant3[k3 + 1] = g;
    quant3[k3 + 2] = b;
  }
}

__global__ void __launch_bounds__(BT) rowCheckKernel(const uint32_t* __restrict__ c4, int w, int* first, int* flags) {
  const int i = blockIdx.x;
  const uint32_t* row = c4 + (size_t)i * w;
  const uint32_t x = row[0] & 0xffffu;
  bool bad = false;
  for (int j = threadIdx.x; j < w; j += BT) bad |= (row[j] & 0xffffu) != x;
  if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(&flags[ENV_ROWS_BAD], 1);
  if (threadIdx.x == 0) atomicMin(&first[x], i);
}

__global__ void __launch_bounds__(SCAN_T) rowIdKernel(const uint32_t* __restrict__ c4, int w, int h, const int* first,
                                                      int* ids, uint32_t* cacheRow, int* flags) {
  __shared__ int part[SCAN_T];
  const int t = threadIdx.x;
  const int per = (h + SCAN_T - 1) / SCAN_T;
  const int lo = min(h, t * per), hi = min(h, lo + per);
  int cnt = 0;
  for (int i = lo; i < hi; i++) cnt += first[c4[(size_t)i * w] & 0xffffu] == i;
  part[t] = cnt;
  __syncthreads();
  for (int off = 1; off < SCAN_T; off <<= 1) {  // inclusive scan of the threads' leader counts
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int id = part[t] - cnt;  // leaders in the rows before this thread's
  for (int i = lo; i < hi; i++)
    if (first[c4[(size_t)i * w] & 0xffffu] == i) ids[i] = id++;
  if (t == SCAN_T - 1) flags[ENV_ROW_IDS] = part[t];
  __syncthreads();  // the block's ids are written: every row reads its leader's
  for (int i = lo; i < hi; i++) {
    const uint32_t x = c4[(size_t)i * w] & 0xffffu;
    cacheRow[i] = x | (uint32_t)ids[first[x]] << 16;
  }
}

__global__ void __launch_bounds__(BT) rowYKernel(const uint32_t* __restrict__ c4, int w, const int* __restrict__ first,
                                                 const uint32_t* __restrict__ cacheRow, unsigned short* cacheY, int* flags) {
  const int i = blockIdx.x;
  const uint32_t r = cacheRow[i];
  const int leader = first[r & 0xffffu];
  const uint32_t* row = c4 + (size_t)i * w;
  bool bad = false;
  if (leader == i) {
    unsigned short* out = cacheY + (size_t)(r >> 16) * w;
    for (int j = threadIdx.x; j < w; j += BT) out[j] = (unsigned short)(row[j] >> 16);
  } else {
    const uint32_t* lead = c4 + (size_t)leader * w;
    for (int j = threadIdx.x; j < w; j += BT) bad |= (row[j] >> 16) != (lead[j] >> 16);
  }
  if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(&flags[ENV_ROWS_BAD], 1);
}

__global__ void __launch_bounds__(BT) envDecodeKernel(Env e, int form, float4* texels, float2* table) {
  const int k = blockIdx.x * BT + threadIdx.x;
  if (k >= e.w * e.h) return;
  if (texels) texels[k] = decodeHdr8(e.hdr8[k]);
  if (!table) return;
  if (form == 1) {
    table[k] = decodeCache4(e.cache4[k], e.w, e.h);
  } else {
    // the frame kernels' own lookup (e.cacheRow is set), aimed at the texel's centre: floor((c + 0.5) / w * w)
    // is c for every c below 2^22
    const int row = k / e.w, col = k - row * e.w;
    table[k] = hdrCacheTexel(e, ((float)col + 0.5f) / (float)e.w, ((float)row + 0.5f) / (float)e.h);
  }
}

inline unsigned blocks(long n) { return (unsigned)((n + BT - 1) / BT); }

}  // namespace

hipError_t launchEnvTexels(const float* src3, const float* cache3, int rgbe, float4* hdr, float2* samp, float* quant3,
                           int n, hipStream_t s) {
  if (!src3 || !hdr || !samp || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(envTexelsKernel, dim3(blocks(n)), dim3(BT), 0, s, src3, cache3, rgbe, hdr, samp, quant3, n);
  return hipGetLastError();
}

hipError_t launchEnvRows(const EnvStore& st, hipStream_t s) {
  if (!st.cache4 || !st.cacheRow || !st.cacheY || !st.rowTmp || !st.flags || st.w < 1 || st.h < 1 || st.w > 65535 ||
      st.h > 65535)
    return hipErrorInvalidValue;
  int* first = st.rowTmp;
  int* ids = st.rowTmp + ENV_X_SLOTS;
  hipError_t e = hipMemsetAsync(first, 0x7f, ENV_X_SLOTS * sizeof(int), s);  // above every row number
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rowCheckKernel, dim3((unsigned)st.h), dim3(BT), 0, s, st.cache4, st.w, first, st.flags);
  hipLaunchKernelGGL(rowIdKernel, dim3(1), dim3(SCAN_T), 0, s, st.cache4, st.w, st.h, first, ids, st.cacheRow, st.flags);
  hipLaunchKernelGGL(rowYKernel, dim3((unsigned)st.h), dim3(BT), 0, s, st.cache4, st.w, first, st.cacheRow, st.cacheY,
                     st.flags);
  return hipGetLastError();
}

hipError_t launchEnvDecode(const Env& e, int form, float4* texels, float2* table, hipStream_t s) {
  if (e.w < 1 || e.h < 1 || (!texels && !table) || (form != 1 && form != 2)) return hipErrorInvalidValue;
  if ((texels && !e.hdr8) || (table && form == 1 && !e.cache4) || (table && form == 2 && (!e.cacheRow || !e.cacheY || !e.cache)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(envDecodeKernel, dim3(blocks((long)e.w * e.h)), dim3(BT), 0, s, e, form, texels, table);
  return hipGetLastError();
}

}  // namespace pt
