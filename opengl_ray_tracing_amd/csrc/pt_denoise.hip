// pt_denoise.hip -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of the running
// mean, steered by the guide buffers (pt_abi.h pt_denoise). One launch per pass; the pass itself is
// pt_atrous.h's tile function with the colour term below. tests/denoise_ref.py is the
// specification: every f32 operation is one of its operations, in its order, so the output equals
// it bit for bit (no fused multiply-adds, IEEE division, ptm_expf shared with the host).
//
// Per pixel a pass reads 5 float4 (colour, tone-mapped colour, position + t, normal + triangle,
// albedo) of 25 taps. tm(c) is computed once per pixel per pass: each pass writes tm(out) beside
// out as a fourth plane for the next pass (atrousTmKernel writes the first pass's from the
// accumulation), so a tap never recomputes it. Staged, a pixel's four float4 are (c.rgb, valid),
// (tm.rgb, A.r), (P.xyz, A.g), (N.xyz, A.b).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_atrous.h"
#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

__global__ void atrousTmKernel(const float4* in, float4* tm, int n, float limit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 t = tonemapPixel(in[i], limit, 0.0f);
  tm[i] = make_float4(t.x, t.y, t.z, 0.0f);
}

// the colour term: |tm(q) - tm(p)|^2 / sigma_c_i^2
struct ColourTerm {
  using Params = AtrousParams;
  using Px = V3;  // tm(c)
  static __device__ __forceinline__ Px load(const Params& p, size_t g) {
    const float4 tm = p.tmIn[g];
    return v3(tm.x, tm.y, tm.z);
  }
  static __device__ __forceinline__ void pack(float4 pos, float4 nrm, float4 alb, Px tm, float4& b, float4& c,
                                              float4& d) {
    b = make_float4(tm.x, tm.y, tm.z, alb.x);
    c = make_float4(pos.x, pos.y, pos.z, alb.y);
    d = make_float4(nrm.x, nrm.y, nrm.z, alb.z);
  }
  static __device__ __forceinline__ void unpack(float4 b, float4 c, float4 d, V3& P, V3& N, V3& A, Px& tm) {
    tm = v3(b.x, b.y, b.z);
    P = v3(c.x, c.y, c.z);
    N = v3(d.x, d.y, d.z);
    A = v3(b.w, c.w, d.w);
  }

  const size_t i;
  V3 Tp;
  bool cOn;
  __device__ __forceinline__ ColourTerm(const Params&, size_t i_) : i(i_) {}
  template <bool STAGE>
  __device__ __forceinline__ void centre(const Params& p, const AtrousAt&, const float4*) {
    Tp = load(p, i);
    cOn = p.colOn != 0;
  }
  __device__ __forceinline__ void range(const Params& p, Px tm, float& a) const {
    if (cOn) {
      const V3 D = tm - Tp;
      a = a + dot(D, D) / p.colDen;
    }
  }
  __device__ __forceinline__ void accumulate(bool, Px, float) {}
  __device__ __forceinline__ void normalise(float) {}
  __device__ __forceinline__ void write(const Params& p, float4 out, bool) const {
    if (p.tmOut) {
      const V3 t = tonemapPixel(out, p.limit, 0.0f);
      p.tmOut[i] = make_float4(t.x, t.y, t.z, 0.0f);
    }
  }
};

template <bool STAGE>
__global__ __launch_bounds__(ATROUS_TILE* ATROUS_TILE) void atrousKernel(AtrousParams p) {
  extern __shared__ __attribute__((aligned(16))) float4 s_px[];
  atrousTile<ColourTerm, STAGE>(p, s_px);
}

hipError_t launchAtrousTm(const float4* in, float4* tm, int n, float limit, hipStream_t s) {
  hipLaunchKernelGGL(atrousTmKernel, dim3((n + 255) / 256), dim3(256), 0, s, in, tm, n, limit);
  return hipGetLastError();
}

hipError_t launchAtrous(const AtrousParams& p, hipStream_t s) {
  return launchAtrousPass(atrousKernel<true>, atrousKernel<false>, p, s);
}

}  // namespace pt
