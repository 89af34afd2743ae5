// pt_diag.hip -- diagnostics: device functions the frame kernels inline, evaluated on inputs a
// test aims (include/pt_fmath.h, pt_device.h sphTexel), for bit-equality with the host.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"

namespace pt {

// include/pt_fmath.h evaluated on the device (diagnostics; bit-equality with the host)
__device__ __forceinline__ float fmathEval(int fn, float x, float y) {
  switch (fn) {
    case 0: return ptm_sinf(x);
    case 1: return ptm_cosf(x);
    case 2: return ptm_atan2f(x, y);
    case 3: return ptm_asinf(x);
    case 4: return ptm_logf(x);
    case 5: return ptm_expf(x);
    case 6: return ptm_powf(x, y);
    case 7: return ptm_atan2f_fast(x, y);
    case 8: return ptm_asinf_fast(x);
    default: {  // 9, 10: the sine and the cosine of ptm_sincosf
      float s, c;
      ptm_sincosf(x, &s, &c);
      return fn == 9 ? s : c;
    }
  }
}
__global__ void fmathKernel(int fn, const float* x, const float* y, int n, float* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = fmathEval(fn, x[i], y ? y[i] : 0.0f);
}
hipError_t launchFmath(int fn, const float* x, const float* y, int n, float* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fmathKernel, dim3((n + 255) / 256), dim3(256), 0, s, fn, x, y, n, out);
  return hipGetLastError();
}
// sphTexel and sphTexelExact (pt_device.h) of n directions taken as they are given (diagnostics: the
// decision the frame kernels inline, at directions a test aims)
__global__ void sphTexelKernel(int W, int H, const float* dirs, int n, int* texel, int* texelExact) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 v = v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
  texel[i] = sphTexel(W, H, v);
  texelExact[i] = sphTexelExact(W, H, v);
}

hipError_t launchSphTexel(int W, int H, const float* dirs, int n, int* texel, int* texelExact, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sphTexelKernel, dim3((n + 255) / 256), dim3(256), 0, s, W, H, dirs, n, texel, texelExact);
  return hipGetLastError();
}

}  // namespace pt
