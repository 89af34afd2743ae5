// pt_paths.h -- the three pass1.fsh integrators from a path's first hit on, and the sum that ends a
// sample. The megakernel (pt_kernels.hip finishPixel, a pixel's camera hit) and the radiance query
// (pt_radiance.hip, a caller's ray) run this one text, so a caller's ray that equals a pixel's camera
// ray yields that pixel's sample bit for bit. T is a pt_trace.h Tracer.
#pragma once
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_trace.h"

namespace pt {

// ------------------------------------------------------------ integrators
// pathTracing O:329-364
template <class T>
__device__ V3 pathLambert(T& tr, const Env& env, Hit hit, int maxBounce, uint32_t& seed, Counters& C, bool count) {
  V3 Lo = v3(0, 0, 0), history = v3(1, 1, 1);
  for (int bounce = 0; bounce < maxBounce; bounce++) {
    V3 wi = toNormalHemisphere(sampleHemisphereRand(seed), hit.N);
    Hit nh;
    bool isHit = tr.closest(hit.P, wi, nh);
    float pdf = 1.0f / (2.0f * PT_PI);
    float cosine_i = fmaxf(0.0f, dot(wi, hit.N));
    V3 f_r = hit.m.baseColor / PT_PI;
    if (!isHit) {
      V3 sky = sampleHdr(env, wi);
      if (count) C.texels++;
      Lo = Lo + ((history * sky) * f_r * cosine_i) / pdf;
      break;
    }
    V3 Le = nh.m.emissive;
    Lo = Lo + ((history * Le) * f_r * cosine_i) / pdf;
    hit = nh;
    history = history * ((f_r * cosine_i) / pdf);
  }
  return Lo;
}

// pathTracing D:443-481
template <class T>
__device__ V3 pathDisneyUniform(T& tr, const Env& env, Hit hit, int maxBounce, uint32_t& seed, Counters& C,
                                bool count) {
  V3 Lo = v3(0, 0, 0), history = v3(1, 1, 1);
  for (int bounce = 0; bounce < maxBounce; bounce++) {
    V3 V = -hit.viewDir;
    V3 N = hit.N;
    V3 L = toNormalHemisphere(sampleHemisphereRand(seed), hit.N);
    float pdf = 1.0f / (2.0f * PT_PI);
    float cosine_i = fmaxf(0.0f, dot(L, N));
    V3 tangent, bitangent;
    getTangent(N, tangent, bitangent);
    V3 f_r = brdfAniso(V, N, L, tangent, bitangent, hit.m);
    Hit nh;
    bool isHit = tr.closest(hit.P, L, nh);
    if (!isHit) {
      V3 sky = sampleHdr(env, L);
      if (count) C.texels++;
      Lo = Lo + ((history * sky) * f_r * cosine_i) / pdf;
      break;
    }
    V3 Le = nh.m.emissive;
    Lo = Lo + ((history * Le) * f_r * cosine_i) / pdf;
    hit = nh;
    history = history * ((f_r * cosine_i) / pdf);
  }
  return Lo;
}

// pathTracingImportanceSampling IS:761-841
//
// Evaluated in a different order from the reference, with the same operations
// on the same values (so the same bits): everything that needs the hit's
// material -- the light sample's contribution and the BRDF sample with its
// f_r and pdf -- is computed before either ray of the bounce is traced, and
// the light contribution is added only if the shadow ray is unoccluded. No
// material, view vector or normal is live across a traversal. Random numbers are
// drawn in the reference's order (r1, r2, then xi_3); the shadow ray is traced and
// counted exactly when the reference traces it. Both rays of a bounce go through
// one traversal call site (Tracer::traceK): the loop's phase says which ray is in
// flight, so a lane whose bounce has no shadow ray walks its BRDF ray beside
// another lane's shadow ray, and the kernel holds one copy of the walk.
template <class T>
__device__ V3 pathMIS(T& tr, const Env& env, Hit hit, int maxBounce, uint32_t& seed, int px, int py,
                      uint32_t frameCounter, Counters& C, bool count) {
  V3 Lo = v3(0, 0, 0), history = v3(1, 1, 1);
  if (maxBounce <= 0) return Lo;
  const uint32_t gi = grayCode(frameCounter + 1u);  // frameCounter = the sample index here
  float cpu, cpv;
  cranleyPattersonShift(px, py, cpu, cpv);
  for (int bounce = 0; bounce < maxBounce; bounce++) {
    const V3 V = -hit.viewDir;
    const V3 N = hit.N;
    // (1) light sample IS:772-789
    const float r1 = randf(seed);
    const float r2 = randf(seed);
    int ent;
    const V3 Ldir = sampleHdrDir(env, r1, r2, &ent);
    if (count) C.texels++;
    const bool tryLight = dot(N, Ldir) > 0.0f;
    V3 lightC = v3(0, 0, 0);
    if (tryLight) {
      V3 color;
      float pdf_light;
      hdrLightColorPdf(env, ent, Ldir, color, pdf_light);
      const V3 fl = brdfIso(V, N, Ldir, hit.m);
      const float pb = brdfPdf(V, N, Ldir, hit.m);
      const float mis_weight = misWeight(pdf_light, pb);
      const V3 c = ((history * mis_weight) * color) * fl;
      lightC = (c * dot(N, Ldir)) / pdf_light;
    }
    // (2) BRDF sample IS:791-840
    float u = sobolf(2u * (uint32_t)bounce, gi);
    float v = sobolf(2u * (uint32_t)bounce + 1u, gi);
    cranleyPattersonApply(cpu, cpv, u, v);
    const float xi_3 = randf(seed);
    const V3 L = sampleBRDF(u, v, xi_3, V, N, hit.m);
    const float NdotL = dot(N, L);
    const V3 f_r = brdfIso(V, N, L, hit.m);
    const float pdf_brdf = brdfPdf(V, N, L, hit.m);
    const V3 P = hit.P;
    if (!tryLight && NdotL <= 0.0f) break;  // IS:818: no ray left in this bounce
    // (3) the bounce's rays, the env shadow ray first when there is one, through one call site
    bool shadow = tryLight, end = false;
    int tri;
    float t;
    while (true) {
      tri = tr.traceK(P, shadow ? Ldir : L, shadow, t);
      if (!shadow) break;
      if (tri < 0) {  // IS:776-790
        Lo = Lo + lightC;
        if (count) C.texels += 2;
      }
      shadow = false;
      if (NdotL <= 0.0f) {
        end = true;
        break;
      }
    }
    if (end) break;
    if (pdf_brdf <= 0.0f) break;  // IS:816: the ray is traced, then discarded
    if (tri < 0) {  // IS:819-829
      V3 color;
      float pdf_light;
      hdrColorPdf(env, L, color, pdf_light);
      if (count) C.texels += 2;
      const float mis_weight = misWeight(pdf_brdf, pdf_light);
      const V3 c = ((history * mis_weight) * color) * f_r;
      Lo = Lo + (c * NdotL) / pdf_brdf;
      break;
    }
    finishHit(tr.S, tri, P, L, t, hit);  // IS:831-840: the next bounce's hit
    const V3 Le = hit.m.emissive;
    Lo = Lo + ((history * Le) * f_r * NdotL) / pdf_brdf;
    history = history * ((f_r * NdotL) / pdf_brdf);
  }
  return Lo;
}

// One sample from a path's first hit (triangle tri at t along (o, d), the RNG state seed as the camera
// ray's jitter left it): the integrator's Li plus the first hit's emission (main IS:853-866), the sum
// pt_kernels.hip finishPixel states. (The megakernel keeps its own statement: routed through this
// function its register use stayed and its code grew by 8-44 bytes per variant)
template <int INTEG, class T>
__device__ __forceinline__ V3 pathSample(T& tr, const Env& env, int tri, V3 o, V3 d, float t, int maxBounce,
                                         uint32_t& seed, int px, int py, uint32_t sampleIndex, Counters& C, bool count) {
  Hit first;
  finishHit(tr.S, tri, o, d, t, first);
  V3 Li;
  if (INTEG == 0) Li = pathLambert(tr, env, first, maxBounce, seed, C, count);
  else if (INTEG == 1) Li = pathDisneyUniform(tr, env, first, maxBounce, seed, C, count);
  else Li = pathMIS(tr, env, first, maxBounce, seed, px, py, sampleIndex, C, count);
  // MIS (8-16 bounces): the camera hit's emission reloaded once the path has ended rather than
  // held across every bounce (the megakernel at its 168-VGPR limit: 37 -> 28 VGPRs spilled)
  const V3 Le0 = INTEG == 2 ? emissiveOf(tr.S, tri) : first.m.emissive;
  return Le0 + Li;
}

}  // namespace pt
