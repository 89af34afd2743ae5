// pt_basic.hip -- the BasicRayTracingWithC++ integrator (pt_abi.h PT_BASIC): one sample of every
// pixel per launch over the reference's shape list, and the widen / narrow kernels of its
// checkpoints. It shares nothing with the frame kernels but the vector type.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_scene.h"

namespace pt {

// ------------------------------------------------ BASIC (BasicRayTracingWithC++)
// The reference binary's arithmetic (oracle/pt_oracle.c b_*, pinned byte for byte
// against the reference compiled from its source): glm vec3 is float, the Material
// rates, the sphere radius, HitResult::distance and the image are double
// (B:49-68, :130, :356), each mixed expression in the type C++ promotes it to.
struct BHit {
  double distance;
  V3 P, N, color;
  bool emissive;
  double specularRate, roughness, refractRate, refractAngle, refractRoughness;
};
// randf B:211-214: the per-pixel counter stream, or the replayed reference stream
struct BRng {
  uint32_t seed;
  const double* rep;
  long long pos, end;
  bool over;
};
__device__ __forceinline__ double bRand(BRng& g) {
  if (g.rep) {
    if (g.pos < g.end) return g.rep[g.pos++];
    g.over = true;
    return 0.5;
  }
  return (double)wang(g.seed) / 4294967296.0;
}
__device__ __forceinline__ V3 ldf3(const double* p) { return v3((float)p[0], (float)p[1], (float)p[2]); }
// Triangle::intersect B:90-122 / Sphere::intersect B:135-164 (OS, SH, t float; pow(x, 2)
// of a float exact in double; R double, so OH > R and PH double expressions)
__device__ __forceinline__ bool bIntersect(const double* sh, V3 S, V3 d, BHit& res) {
  if (sh[0] == 1.0) {
    V3 O = ldf3(sh + 1);
    double R = sh[22];
    V3 OSv = O - S;
    float OS = sqrtf(dot(OSv, OSv));
    float SH = dot(OSv, d);
    float OH = (float)sqrt((double)OS * (double)OS - (double)SH * (double)SH);
    if ((double)OH > R) return false;
    float PH = (float)sqrt(R * R - (double)OH * (double)OH);
    float t1 = fabsf(SH) - PH;
    float t2 = fabsf(SH) + PH;
    float t = (t1 < 0) ? t2 : t1;
    V3 P = S + d * t;
    if (fabsf(t1) < 0.0005f || fabsf(t2) < 0.0005f) return false;
    res.distance = t;
    res.P = P;
    res.N = normalize(P - O);
  } else {
    V3 p1 = ldf3(sh + 1), p2 = ldf3(sh + 4), p3 = ldf3(sh + 7), n = ldf3(sh + 13);
    V3 N = n;
    if (dot(N, d) > 0.0f) N = -N;
    if (fabsf(dot(N, d)) < 0.00001f) return false;
    float t = (dot(N, p1) - dot(S, N)) / dot(d, N);
    if (t < 0.0005f) return false;
    V3 P = S + d * t;
    V3 c1 = cross(p2 - p1, P - p1), c2 = cross(p3 - p2, P - p2), c3 = cross(p1 - p3, P - p3);
    if (dot(c1, n) < 0 || dot(c2, n) < 0 || dot(c3, n) < 0) return false;
    res.distance = t;
    res.P = P;
    res.N = N;
  }
  res.color = ldf3(sh + 10);
  res.emissive = sh[16] != 0.0;
  res.specularRate = sh[17]; res.roughness = sh[18]; res.refractRate = sh[19];
  res.refractAngle = sh[20]; res.refractRoughness = sh[21];
  return true;
}
// shoot B:192-205 (res.distance a double initialised from 1145141919.810f)
__device__ __forceinline__ bool bShoot(const double* shapes, int n, V3 S, V3 d, BHit& best) {
  bool any = false;
  best.distance = (double)1145141919.810f;
  for (int k = 0; k < n; k++) {
    BHit r;
    if (bIntersect(shapes + (size_t)k * PT_SHAPE_DOUBLES, S, d, r) && r.distance < best.distance) {
      best = r;
      any = true;
    }
  }
  return any;
}
// randomVec3 B:217-234 (the compiled reference evaluates vec3(randf(), randf(), randf())
// right to left: z takes the first draw) / randomDirection B:237-250
__device__ __forceinline__ V3 bRandomDirection(V3 n, BRng& g) {
  V3 dd;
  do {
    double z = bRand(g), y = bRand(g), x = bRand(g);
    dd = v3((float)x, (float)y, (float)z) * 2.0f - v3(1, 1, 1);
  } while ((double)dot(dd, dd) > 1.0);
  return normalize(normalize(dd) + n);
}
// glm reflect / refract (func_geometric.inl:104-123), glm mix(vec3, vec3, double) in double
__device__ __forceinline__ V3 bReflect(V3 I, V3 N) { return I - (N * dot(N, I)) * 2.0f; }
__device__ __forceinline__ V3 bRefract(V3 I, V3 N, float eta) {
  float dv = dot(N, I);
  float k = 1.0f - eta * eta * (1.0f - dv * dv);
  if (!(k >= 0.0f)) return v3(0, 0, 0);
  return I * eta - N * (eta * dv + sqrtf(k));
}
__device__ __forceinline__ V3 bMixd(V3 x, V3 y, double a) {
  const double b = 1.0 - a;
  return v3((float)((double)x.x * b + (double)y.x * a), (float)((double)x.y * b + (double)y.y * a),
            (float)((double)x.z * b + (double)y.z * a));
}
// lobe choice + new direction (B:399-422, B:268-294): 0 specular, 1 refract, 2 diffuse
__device__ __forceinline__ int bLobe(const BHit& res, V3 din, BRng& g, V3& dout) {
  V3 rd = bRandomDirection(res.N, g);
  double r = bRand(g);
  if (r < res.specularRate) {
    dout = bMixd(normalize(bReflect(din, res.N)), rd, res.roughness);
    return 0;
  } else if (res.specularRate <= r && r <= res.refractRate) {
    dout = bMixd(normalize(bRefract(din, res.N, (float)res.refractAngle)), -rd, res.refractRoughness);
    return 1;
  }
  dout = rd;
  return 2;
}

__global__ __launch_bounds__(BLOCK) void basicKernel(BasicParams p) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15);
  const int i = blockIdx.y * 16 + (threadIdx.x >> 4);
  uint32_t rays = 0;
  bool over = false;
  if (j < p.width && i < p.height) {
    const int W = p.width, H = p.height;
    BRng g;
    g.seed = ((uint32_t)j * 1973u + (uint32_t)i * 9277u + p.sample * 26699u + p.seed * 0x9E3779B9u) | 1u;
    g.rep = p.stream;
    g.pos = g.end = 0;
    g.over = false;
    if (p.stream) {
      const long long idx = ((long long)p.sample * H + i) * W + j;
      if (idx < p.nOffsets) {
        g.pos = p.offsets[idx];
        g.end = idx + 1 < p.nOffsets ? p.offsets[idx + 1] : p.streamN;
        g.end = g.end < p.streamN ? g.end : p.streamN;
      }
    }
    // pixel loop body B:367-429
    double xd = 2.0 * (double)j / (double)W - 1.0;
    double yd = 2.0 * (double)(H - i) / (double)H - 1.0;
    xd += (bRand(g) - 0.5) / (double)W;
    yd += (bRand(g) - 0.5) / (double)H;
    V3 coord = v3((float)xd, (float)yd, (float)1.1);  // SCREEN_Z B:27 is a double
    V3 dir = normalize(coord - v3(0, 0, 4.0f));
    BHit res;
    V3 color = v3(0, 0, 0);
    rays++;
    if (bShoot(p.shapes, p.nShapes, coord, dir, res)) {
      if (res.emissive) {
        color = res.color;
      } else {
        V3 nd;
        int lobe = bLobe(res, dir, g, nd);
        // pathTracing B:252-297 from depth 0: the recursion forms its products on the way
        // back up (pathTracing(depth + 1) * cosine [* srcColor] / P), so each vertex's
        // factors are kept and folded from the deepest vertex upward
        float cosv[BASIC_MAX_DEPTH + 1];
        V3 col[BASIC_MAX_DEPTH + 1];
        bool diff[BASIC_MAX_DEPTH + 1];
        const float P = 0.8f;  // B:264
        V3 S = res.P, d = nd, v = v3(0, 0, 0);
        int n = 0;
        for (int depth = 0; depth <= p.maxDepth; depth++) {
          BHit h;
          rays++;
          if (!bShoot(p.shapes, p.nShapes, S, d, h)) break;
          if (h.emissive) { v = h.color; break; }
          double r = bRand(g);
          if (r > (double)P) break;
          V3 nd2;
          int lb = bLobe(h, d, g, nd2);
          cosv[n] = fabsf(dot(-d, h.N));
          col[n] = h.color;
          diff[n] = lb == 2;
          n++;
          S = h.P;
          d = nd2;
        }
        for (int k = n - 1; k >= 0; k--) {
          v = v * cosv[k];
          if (diff[k]) v = v * col[k];
          v = v / P;
        }
        color = (lobe == 2) ? v * res.color : v;
        color = color * p.brightness;  // color *= BRIGHTNESS (glm casts the double to float)
      }
    }
    double* im = p.image + 3 * ((size_t)i * W + j);
    double r0 = p.reset ? 0.0 : im[0], r1 = p.reset ? 0.0 : im[1], r2 = p.reset ? 0.0 : im[2];
    r0 += color.x; r1 += color.y; r2 += color.z;  // *p += color.x ... (B:427-429)
    im[0] = r0; im[1] = r1; im[2] = r2;
    p.accum[(size_t)i * W + j] = make_float4((float)r0, (float)r1, (float)r2, 1.0f);
    over = g.over;
  }
  // wave-reduce the ray count, one atomic per wave
  for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off, 64);
  if ((threadIdx.x & 63) == 0 && rays) atomicAdd(reinterpret_cast<unsigned long long*>(p.stats), (unsigned long long)rays);
  const unsigned long long ov = __ballot(over);
  if ((threadIdx.x & 63) == 0 && ov) atomicAdd(p.overruns, (unsigned long long)__popcll(ov));
}

hipError_t launchBasic(const BasicParams& p, hipStream_t s) {
  dim3 grid((p.width + 15) / 16, (p.height + 15) / 16);
  hipLaunchKernelGGL(basicKernel, grid, dim3(BLOCK), 0, s, p);
  return hipGetLastError();
}

__global__ void basicWidenKernel(const float4* accum, double* image, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = accum[i];
  image[3 * i] = (double)a.x;
  image[3 * i + 1] = (double)a.y;
  image[3 * i + 2] = (double)a.z;
}
__global__ void basicNarrowKernel(const double* image, float4* accum, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  accum[i] = make_float4((float)image[3 * i], (float)image[3 * i + 1], (float)image[3 * i + 2], 1.0f);  // basicKernel's store
}
hipError_t launchBasicWiden(const float4* accum, double* image, long n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(basicWidenKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, accum, image, n);
  return hipGetLastError();
}
hipError_t launchBasicNarrow(const double* image, float4* accum, long n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(basicNarrowKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, image, accum, n);
  return hipGetLastError();
}

}  // namespace pt
