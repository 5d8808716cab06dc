// phong.h -- per-fragment Phong lighting of PyTorch3D's SoftPhongShader (phong_shading / PointLights.diffuse / .specular),
// forward and hand-written backward, shared by the specialised K = 1 kernels (shade.hip) and the general soft kernels
// (soft.hip).  Everything is in world space:
//   N = sum_i b_i n_{f,i} (vertex normals, not renormalised), P = sum_i b_i v_{f,i}, C = -T R^T (camera centre)
//   L = location - P (point) | direction (directional);  n = N / max(|N|, 1e-6), l = L / max(|L|, 1e-6)
//   cos = n.l;  D = kd Ld relu(cos);  r = -l + 2 cos n;  e = normalize(C - P);  alpha = relu(e.r) [cos > 0]
//   Sp = ks Ls alpha^shininess;  A = ka La;  colour = (A + D) texel + Sp
// relu is __builtin_elementwise_maximum (NaN stays NaN, as torch.relu) and the gate is written !(cos <= 0): a NaN anywhere
// reaches the colour instead of being laundered into 0 by fmaxf.
//
// Light block (include/st3d.h): per entry kLightFloats floats
//   [0..2] ambient_color  [3..5] diffuse_color  [6..8] specular_color  [9..11] location (point) / direction
//   [12..14] material ambient  [15..17] material diffuse  [18..20] material specular  [21] shininess  [22..23] unused
// n_lights == 1: every view uses entry 0; otherwise view b uses entry b.
#pragma once
#include "common.h"

namespace st3d_phong {

constexpr int kLightFloats = 24;
constexpr float kNormEps = 1e-6f;

// kind: which light the block describes
enum { kAmbient = 0, kPoint = 1, kDirectional = 2, kHeadlight = 3 };   // kHeadlight: a point light at the view's camera centre

struct LitArgs {
    const float *verts, *normals;       // (V,3) world positions and vertex normals (unused for kAmbient)
    const int32_t *faces;               // (F,3)
    const float *R, *T;                 // (B,3,3), (B,3): camera of every view
    const float *light;                 // n_lights x kLightFloats
    int n_lights, kind;
    float *grad_np;                     // backward: per fragment d/dN (3) and d/dP (3), or nullptr
};

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(const float *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 operator*(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float relu(float x) { return __builtin_elementwise_maximum(x, 0.0f); }

// x / max(|x|, eps) and its backward (g_x = (g - x^ (x^.g)) / |x|, or g / eps below the eps)
__device__ __forceinline__ F3 normalize(F3 x) { return x * (1.0f / __builtin_elementwise_maximum(sqrtf(dot3(x, x)), kNormEps)); }
__device__ __forceinline__ F3 normalize_bwd(F3 x, F3 g) {
    const float len = sqrtf(dot3(x, x));
    if (!(len > kNormEps)) return g * (1.0f / kNormEps);
    const F3 xh = x * (1.0f / len);
    return (g - xh * dot3(xh, g)) * (1.0f / len);
}

__device__ __forceinline__ const float *entry(const LitArgs &la, int b) {
    return la.light + (size_t)(la.n_lights == 1 ? 0 : b) * kLightFloats;
}

// camera centre of view b: X_view = X R + T = 0  =>  C_j = -sum_k T_k R_jk
__device__ __forceinline__ F3 camera_centre(const LitArgs &la, int b) {
    const float *R = la.R + (size_t)b * 9, *T = la.T + (size_t)b * 3;
    return {-(T[0] * R[0] + T[1] * R[1] + T[2] * R[2]), -(T[0] * R[3] + T[1] * R[4] + T[2] * R[5]),
            -(T[0] * R[6] + T[1] * R[7] + T[2] * R[8])};
}

// the interpolated normal and position of fragment (face f, barycentrics b0 b1 b2)
__device__ __forceinline__ void interpolate(const LitArgs &la, int f, float b0, float b1, float b2, F3 &N, F3 &P) {
    const int i0 = la.faces[3 * f], i1 = la.faces[3 * f + 1], i2 = la.faces[3 * f + 2];
    N = (f3(la.normals + 3 * i0) * b0 + f3(la.normals + 3 * i1) * b1) + f3(la.normals + 3 * i2) * b2;
    P = (f3(la.verts + 3 * i0) * b0 + f3(la.verts + 3 * i1) * b1) + f3(la.verts + 3 * i2) * b2;
}

__device__ __forceinline__ F3 light_vector(const LitArgs &la, const float *L, F3 P, F3 C) {
    if (la.kind == kDirectional) return f3(L + 9);
    return (la.kind == kHeadlight ? C : f3(L + 9)) - P;
}

// colour_c = ad[c] * texel_c + sp[c]
__device__ __forceinline__ void phong_fwd(const LitArgs &la, int b, int f, float b0, float b1, float b2, float ad[3], float sp[3]) {
    const float *L = entry(la, b);
    if (la.kind == kAmbient) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { ad[c] = L[12 + c] * L[c]; sp[c] = 0.f; }
        return;
    }
    F3 N, P;
    interpolate(la, f, b0, b1, b2, N, P);
    const F3 C = camera_centre(la, b);
    const F3 n = normalize(N), l = normalize(light_vector(la, L, P, C));
    const float cs = dot3(n, l);
    const F3 r = l * -1.0f + n * (2.0f * cs);
    const F3 e = normalize(C - P);
    const float alpha = relu(dot3(e, r)) * (!(cs <= 0.f) ? 1.0f : 0.0f);
    const float dif = relu(cs), spec = powf(alpha, L[21]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ad[c] = L[12 + c] * L[c] + L[15 + c] * L[3 + c] * dif;
        sp[c] = L[18 + c] * L[6 + c] * spec;
    }
}

// upstream d/d(ad), d/d(sp) -> d/dN, d/dP of the fragment (point / directional / headlight only)
__device__ __forceinline__ void phong_bwd(const LitArgs &la, int b, int f, float b0, float b1, float b2, const float g_ad[3],
                                          const float g_sp[3], F3 &gN, F3 &gP) {
    const float *L = entry(la, b);
    F3 N, P;
    interpolate(la, f, b0, b1, b2, N, P);
    const F3 C = camera_centre(la, b);
    const F3 Lv = light_vector(la, L, P, C), E = C - P;
    const F3 n = normalize(N), l = normalize(Lv), e = normalize(E);
    const float cs = dot3(n, l);
    const F3 r = l * -1.0f + n * (2.0f * cs);
    const float er = dot3(e, r);
    const float gate = !(cs <= 0.f) ? 1.0f : 0.0f;
    const float alpha = relu(er) * gate;
    const float sh = L[21];
    float gdif = 0.f, gspec = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gdif += g_ad[c] * (L[15 + c] * L[3 + c]);
        gspec += g_sp[c] * (L[18 + c] * L[6 + c]);
    }
    // spec = alpha^sh (torch.pow backward: sh * alpha^(sh - 1)); alpha = relu(er) * gate; relu passes where its output > 0
    const float galpha = gspec * (sh * powf(alpha, sh - 1.0f));
    const float ger = (er > 0.f) ? galpha * gate : 0.f;
    float gcs = (cs > 0.f) ? gdif : 0.f;
    const F3 ge = r * ger, gr = e * ger;
    // r = -l + 2 cs n
    F3 gl = gr * -1.0f;
    F3 gn = gr * (2.0f * cs);
    gcs += 2.0f * dot3(gr, n);
    gn = gn + l * gcs;
    gl = gl + n * gcs;
    gN = normalize_bwd(N, gn);
    gP = normalize_bwd(E, ge) * -1.0f;
    if (la.kind != kDirectional) gP = gP - normalize_bwd(Lv, gl);
}

}  // namespace st3d_phong
