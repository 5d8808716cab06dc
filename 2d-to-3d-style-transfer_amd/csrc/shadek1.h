// shadek1.h -- the fragment arithmetic every K = 1 shading kernel shares (shade.hip, mipmap.hip, vcolor.hip; soft.hip takes
// the footprint; cover.hip marks the footprint's texels): the UV position of a fragment, the bilinear footprint of a UV
// position and the softmax blend of one fragment against the background.
// The kernels of these files, oracle/raster_ref.c and the numpy restatements of the tests agree bit for bit, so the
// expressions below ARE the roundings: their order and parenthesisation are part of the contract, and every including
// file builds with -ffp-contract=off and the correctly rounded division (build.py).
#pragma once

namespace st3d_k1 {

constexpr float kSigma = 1e-4f, kGamma = 1e-4f, kBlendEps = 1e-10f, kZnear = 1.0f, kZfar = 100.0f;

struct Footprint {
    int x0, x1, r0, r1;
    float wx0, wx1, wy0, wy1;
    bool vx0, vx1, vy0, vy1, cx, cy;
    float ix, iy;                        // the clamped continuous indices (unflipped frame): what the mip levels start from
};

// UV -> bilinear footprint in ORIGINAL texture rows: grid = uv*2-1, map flipped vertically,
// grid_sample(bilinear, align_corners=True, padding_mode='border').
__device__ __forceinline__ Footprint uv_footprint(float u, float v, int T) {
    Footprint o;
    const float gx = u * 2.0f - 1.0f, gy = v * 2.0f - 1.0f;
    float ix = ((gx + 1.0f) / 2.0f) * (float)(T - 1);
    float iy = ((gy + 1.0f) / 2.0f) * (float)(T - 1);
    o.cx = false; o.cy = false;
    if (!(ix >= 0.f)) { ix = 0.f; o.cx = true; } else if (ix > (float)(T - 1)) { ix = (float)(T - 1); o.cx = true; }
    if (!(iy >= 0.f)) { iy = 0.f; o.cy = true; } else if (iy > (float)(T - 1)) { iy = (float)(T - 1); o.cy = true; }
    const float fx = floorf(ix), fy = floorf(iy);
    o.x0 = (int)fx; o.x1 = o.x0 + 1;
    const int yf0 = (int)fy, yf1 = yf0 + 1;
    o.wx1 = ix - fx; o.wx0 = 1.0f - o.wx1;
    o.wy1 = iy - fy; o.wy0 = 1.0f - o.wy1;
    o.vx0 = o.x0 >= 0 && o.x0 < T; o.vx1 = o.x1 >= 0 && o.x1 < T;
    o.vy0 = yf0 >= 0 && yf0 < T;   o.vy1 = yf1 >= 0 && yf1 < T;
    o.r0 = (T - 1) - yf0; o.r1 = (T - 1) - yf1;
    o.ix = ix; o.iy = iy;
    return o;
}

// The UV position of a fragment on face f: its barycentrics over the face's three UV corners, the products added from left
// to right (oracle/raster_ref.c spells the same sum).  u0..u2: the corners' rows of verts_uvs, which the backwards read again.
struct FragUV { int u0, u1, u2; float u, v; };

__device__ __forceinline__ FragUV frag_uv(const float *__restrict__ uvs, const int32_t *__restrict__ fuv, int f, float b0,
                                          float b1, float b2) {
    FragUV o;
    o.u0 = fuv[3 * f]; o.u1 = fuv[3 * f + 1]; o.u2 = fuv[3 * f + 2];
    o.u = b0 * uvs[2 * o.u0] + b1 * uvs[2 * o.u1] + b2 * uvs[2 * o.u2];
    o.v = b0 * uvs[2 * o.u0 + 1] + b1 * uvs[2 * o.u1 + 1] + b2 * uvs[2 * o.u2 + 1];
    return o;
}

struct Blend { float prob, wnum, delta, denom; };

__device__ __forceinline__ Blend blend_k1(float dist, float z) {
    Blend o;
    o.prob = 1.0f / (1.0f + expf(dist / kSigma));
    const float z_inv = (kZfar - z) / (kZfar - kZnear);
    const float z_max = fmaxf(z_inv, kBlendEps);
    o.wnum = o.prob * expf((z_inv - z_max) / kGamma);
    o.delta = fmaxf(expf((kBlendEps - z_max) / kGamma), kBlendEps);
    o.denom = o.wnum + o.delta;
    return o;
}

}  // namespace st3d_k1
