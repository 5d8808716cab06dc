// atlas.h -- the texel of a fragment in a per-face texel atlas (PyTorch3D TexturesAtlas.sample_textures, restated): every
// face owns an R x R block, the lower-left triangle of which (x + y < R) holds the texels whose sub-triangles point with the
// face and the rest, read back to front, those that point against it.  One function for the two kernels of atlas.hip and
// the host entry point st3d_atlas_texel_index; the numpy restatement of the tests agrees with it index for index, so the
// expressions ARE the roundings: fp32, in this order, uncontracted (build.py).
#pragma once

// b0, b1: the fragment's first two barycentrics as rasterised; 1 <= R <= 64 -> the row wy and column wx of its texel.
// The clamp is applied in float before the conversion (a NaN fails `t > 0` and becomes 0), so no bit pattern of b indexes
// outside the block and no out-of-range float -> int conversion happens.
__host__ __device__ inline void atlas_texel_index(float b0, float b1, int R, int &wy, int &wx) {
    const float fr = (float)R, top = (float)(R - 1);
    float t0 = b0 * fr;
    t0 = (t0 > 0.f) ? t0 : 0.f;
    t0 = (t0 < top) ? t0 : top;
    float t1 = b1 * fr;
    t1 = (t1 > 0.f) ? t1 : 0.f;
    t1 = (t1 < top) ? t1 : top;
    wx = (int)t0;
    wy = (int)t1;
    const float s = (b0 + b1) * fr;
    const bool below = (s - (float)(wx + wy)) <= 1.0f;
    if (!below) { wx = R - 1 - wx; wy = R - 1 - wy; }
}
