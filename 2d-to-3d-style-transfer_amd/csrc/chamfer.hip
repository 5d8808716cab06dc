// chamfer.hip -- the surface-to-surface anchor of optimization_target 'mesh'/'both': PyTorch3D's
// sample_points_from_meshes followed by chamfer_distance(knn_points(K=1)), for ONE mesh and ONE pair of clouds.
//   face_area_cdf       fp64 face areas from the fp32 vertices and their inclusive scan in a fixed tree
//   sample_points       inverse-CDF face draw from sorted uniforms (binary search), fp32 barycentric points; the backward
//                       stages one (3,3) block per face (its samples found by binary search in the ascending face_idx, added
//                       in order) and gathers per vertex over the static vertex -> face * 3 + corner CSR
//   knn1                the hot kernel: all-pairs nearest neighbour, one query per lane in registers, y staged in LDS
//                       tiles read by broadcast, the y range split over `segments` workgroups along grid.y; a second pass
//                       takes the minimum over the segments in ascending order, so the lowest index wins among equals
//   chamfer_sum / bwd   ordered fp64 sum of dist^2; the gradient of one side, its inverse list given as a stable sort
// Every sum is taken in a fixed order in fp64 and rounded once: no float atomics anywhere, two runs are bit-equal.
// Built with -ffp-contract=off: the fp32 roundings are the ones written here, the numpy restatement repeats them.
#include "common.h"

namespace {

constexpr int KNN_THREADS = 256;
// Queries per lane (one LDS read serves KQ distance evaluations), tile and grid were measured, kernel alone, on the MI355X:
//   20 000^2, ms:  KQ 1 / 2 / 4 / 8 at 1 024 workgroups wanted 0.130 / 0.115 / 0.132 / 0.125, at 4 096 wanted 0.103 / 0.105 /
//                  0.111 / 0.125; a 1 024-point tile 0.153; 64-thread workgroups 0.133 at best
//    5 000^2, ms:  KQ 1 / 2 / 4 / 8 = 0.013 / 0.017 / 0.031 / 0.061 whatever is wanted (the tiles run out: 20 segments)
// At the sizes the term runs at the search is short of waves, not of LDS bandwidth: several queries per lane only thin the
// grid, so one query per lane and as many segments as bring the grid to 4 096 workgroups.
constexpr int KNN_KQ = 1;                              // queries per lane
constexpr int KNN_QBLOCK = KNN_THREADS * KNN_KQ;       // queries per workgroup
constexpr int KNN_TILE = 256;                          // y points per LDS tile (4 KiB as float4)
constexpr int KNN_TARGET_WG = 4096;                    // workgroups wanted: four workgroups on every SIMD of the chip
constexpr int MAX_POINTS = 1 << 20;
constexpr int SCAN_BLOCK = 1024;

inline int knn_segments(int P1, int P2, int *seg_tiles) {
    const int qblocks = st3d::cdiv(P1, KNN_QBLOCK), ntiles = st3d::cdiv(P2, KNN_TILE);
    int want = KNN_TARGET_WG / qblocks;
    if (want < 1) want = 1;
    if (want > ntiles) want = ntiles;
    const int segments = st3d::cdiv(ntiles, st3d::cdiv(ntiles, want));
    *seg_tiles = st3d::cdiv(ntiles, segments);         // segment length = seg_tiles * KNN_TILE points
    return segments;
}

// d = (dx dx + dy dy) + dz dz, the one distance of this file
__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// grid (qblocks, segments).  Thread t holds queries q0 + t + k * 256, k < KQ.  seg_best / seg_idx: (segments, P1).
// A NaN distance never passes d < best, so a NaN target is never chosen and a NaN query keeps (Inf, 0).
__global__ __launch_bounds__(KNN_THREADS) void knn1_kernel(const float *__restrict__ x, const float *__restrict__ y, int P1, int P2,
                                                           int seg_tiles, float *__restrict__ seg_best, int32_t *__restrict__ seg_idx) {
    __shared__ float4 tile[KNN_TILE];
    const int q0 = blockIdx.x * KNN_QBLOCK + threadIdx.x;
    float qx[KNN_KQ], qy[KNN_KQ], qz[KNN_KQ], best[KNN_KQ];
    int bi[KNN_KQ];
#pragma unroll
    for (int k = 0; k < KNN_KQ; ++k) {
        const int q = q0 + k * KNN_THREADS;
        const bool in = q < P1;
        qx[k] = in ? x[3 * (size_t)q] : 0.f;
        qy[k] = in ? x[3 * (size_t)q + 1] : 0.f;
        qz[k] = in ? x[3 * (size_t)q + 2] : 0.f;
        best[k] = __builtin_inff();
        bi[k] = 0;
    }
    const long seg_lo = (long)blockIdx.y * seg_tiles * KNN_TILE;
    long seg_hi = seg_lo + (long)seg_tiles * KNN_TILE;
    if (seg_hi > P2) seg_hi = P2;
    for (long j0 = seg_lo; j0 < seg_hi; j0 += KNN_TILE) {          // uniform over the workgroup
        const int n = (int)(seg_hi - j0 < KNN_TILE ? seg_hi - j0 : KNN_TILE);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const size_t j = (size_t)j0 + threadIdx.x;
            tile[threadIdx.x] = make_float4(y[3 * j], y[3 * j + 1], y[3 * j + 2], 0.f);
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float4 p = tile[j];                              // every lane reads the same address: a broadcast
#pragma unroll
            for (int k = 0; k < KNN_KQ; ++k) {
                const float d = dist2(qx[k], qy[k], qz[k], p.x, p.y, p.z);
                if (d < best[k]) { best[k] = d; bi[k] = (int)j0 + j; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KNN_KQ; ++k) {
        const int q = q0 + k * KNN_THREADS;
        if (q < P1) {
            seg_best[(size_t)blockIdx.y * P1 + q] = best[k];
            seg_idx[(size_t)blockIdx.y * P1 + q] = bi[k];
        }
    }
}

// minimum over the segments in ascending order with the same d < best; the distance written is recomputed from x_i, y[idx]
__global__ __launch_bounds__(256) void knn1_merge_kernel(const float *__restrict__ x, const float *__restrict__ y, int P1, int P2,
                                                         int segments, const float *__restrict__ seg_best,
                                                         const int32_t *__restrict__ seg_idx, int32_t *__restrict__ idx,
                                                         float *__restrict__ dist) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P1) return;
    float best = __builtin_inff();
    int bi = 0;
    for (int s = 0; s < segments; ++s) {
        const float d = seg_best[(size_t)s * P1 + q];
        if (d < best) { best = d; bi = seg_idx[(size_t)s * P1 + q]; }
    }
    if ((unsigned)bi >= (unsigned)P2) bi = 0;                       // cannot happen; keeps the gather below in bounds
    idx[q] = bi;
    dist[q] = dist2(x[3 * (size_t)q], x[3 * (size_t)q + 1], x[3 * (size_t)q + 2], y[3 * (size_t)bi], y[3 * (size_t)bi + 1],
                    y[3 * (size_t)bi + 2]);
}

// ---------------------------------------------------------------------------------------------------- area CDF
// inclusive scan of one block of SCAN_BLOCK values in LDS (Hillis-Steele: the tree depends on the index alone)
__device__ __forceinline__ double block_scan(double v, double *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < SCAN_BLOCK; o <<= 1) {
        const double a = (int)threadIdx.x >= o ? s[threadIdx.x - o] : 0.0;
        __syncthreads();
        if ((int)threadIdx.x >= o) s[threadIdx.x] += a;
        __syncthreads();
    }
    return s[threadIdx.x];
}

// cdf[f] = the scan of the areas inside block f / SCAN_BLOCK; totals[block] = its sum
__global__ __launch_bounds__(SCAN_BLOCK) void area_scan_kernel(const float *__restrict__ v, const int32_t *__restrict__ faces, int F,
                                                               double *__restrict__ cdf, double *__restrict__ totals) {
    __shared__ double s[SCAN_BLOCK];
    const int f = blockIdx.x * SCAN_BLOCK + threadIdx.x;
    double area = 0.0;
    if (f < F) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const double ax = v[3 * i0], ay = v[3 * i0 + 1], az = v[3 * i0 + 2];
        const double ux = (double)v[3 * i1] - ax, uy = (double)v[3 * i1 + 1] - ay, uz = (double)v[3 * i1 + 2] - az;
        const double wx = (double)v[3 * i2] - ax, wy = (double)v[3 * i2 + 1] - ay, wz = (double)v[3 * i2 + 2] - az;
        const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
        area = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    }
    const double inc = block_scan(area, s);
    if (f < F) cdf[f] = inc;
    if (threadIdx.x == SCAN_BLOCK - 1) totals[blockIdx.x] = inc;
}

// one workgroup: totals[b] <- sum of totals[0..b) (exclusive), SCAN_BLOCK blocks at a time with a carry
__global__ __launch_bounds__(SCAN_BLOCK) void totals_scan_kernel(double *__restrict__ totals, int nb) {
    __shared__ double s[SCAN_BLOCK];
    double carry = 0.0;
    for (int b0 = 0; b0 < nb; b0 += SCAN_BLOCK) {
        const int b = b0 + threadIdx.x;
        const double t = b < nb ? totals[b] : 0.0;
        block_scan(t, s);
        if (b < nb) totals[b] = carry + (threadIdx.x ? s[threadIdx.x - 1] : 0.0);
        const double last = s[SCAN_BLOCK - 1];
        __syncthreads();
        carry += last;
    }
}

__global__ __launch_bounds__(256) void cdf_offset_kernel(double *__restrict__ cdf, const double *__restrict__ totals, int F) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < F && f >= SCAN_BLOCK) cdf[f] = totals[f / SCAN_BLOCK] + cdf[f];
}

// ---------------------------------------------------------------------------------------------------- sampling
__device__ __forceinline__ void bary_weights(const float *__restrict__ r, int N, int n, float &w0, float &w1, float &w2) {
    const float s = sqrtf(r[(size_t)N + n]), r2 = r[2 * (size_t)N + n];
    w0 = 1.0f - s;
    w1 = s * (1.0f - r2);
    w2 = s * r2;
}

__global__ __launch_bounds__(256) void sample_fwd_kernel(const float *__restrict__ v, const int32_t *__restrict__ faces, int F,
                                                         const double *__restrict__ cdf, const float *__restrict__ r, int N,
                                                         float *__restrict__ points, int32_t *__restrict__ face_idx) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double total = cdf[F - 1];
    const double u = (double)r[n] * total;
    int lo = 0, hi = F;                                            // the smallest f with cdf_f > u; a NaN compares false
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    const int f = lo < F ? lo : F - 1;
    float w0, w1, w2;
    bary_weights(r, N, n, w0, w1, w2);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    // a total area that is NaN or Inf (a NaN / Inf vertex somewhere) draws no face: every point is NaN, so the loss is too
    const bool finite = total - total == 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        points[3 * (size_t)n + c] = finite ? (w0 * v[3 * i0 + c] + w1 * v[3 * i1 + c]) + w2 * v[3 * i2 + c] : __builtin_nanf("");
    face_idx[n] = f;
}

// per face: block[corner][coordinate] = sum over its samples, ascending, of w_corner * g in fp64
__global__ __launch_bounds__(256) void sample_bwd_face_kernel(const float *__restrict__ g, const float *__restrict__ r,
                                                              const int32_t *__restrict__ face_idx, int N, int F,
                                                              double *__restrict__ blocks) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int lo = 0, hi = N;                                            // the first n with face_idx[n] >= f
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (face_idx[mid] >= f) hi = mid; else lo = mid + 1;
    }
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int n = lo; n < N && face_idx[n] == f; ++n) {
        float w[3];
        bary_weights(r, N, n, w[0], w[1], w[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) a[3 * k + c] += (double)w[k] * (double)g[3 * (size_t)n + c];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) blocks[9 * (size_t)f + i] = a[i];
}

// per vertex: grad += the blocks of its (face, corner) entries in list order, summed in fp64, rounded once
__global__ __launch_bounds__(256) void sample_bwd_vertex_kernel(const double *__restrict__ blocks, const int32_t *__restrict__ off,
                                                                const int32_t *__restrict__ ref, int V, int F,
                                                                float *__restrict__ grad) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= V) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int q = off[k]; q < off[k + 1]; ++q) {
        const int e = ref[q];
        if ((unsigned)e >= (unsigned)(3 * F)) continue;            // a list of another mesh: nothing is read out of bounds
        sx += blocks[3 * (size_t)e]; sy += blocks[3 * (size_t)e + 1]; sz += blocks[3 * (size_t)e + 2];
    }
    grad[3 * k] += (float)sx; grad[3 * k + 1] += (float)sy; grad[3 * k + 2] += (float)sz;
}

// ---------------------------------------------------------------------------------------------------- chamfer
// one workgroup: out = (float)((double)out + scale * sum_i d[i]); thread t sums i = t, t + 1024, ... then a fixed tree
__global__ __launch_bounds__(SCAN_BLOCK) void chamfer_sum_kernel(const float *__restrict__ d, int P, double scale,
                                                                 float *__restrict__ out) {
    __shared__ double s[SCAN_BLOCK];
    double a = 0.0;
    for (int i = threadIdx.x; i < P; i += SCAN_BLOCK) a += (double)d[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int o = SCAN_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)((double)out[0] + scale * s[0]);
}

// grad_x_i += c_self (x_i - y_nn(i)) + c_other sum_{j: nn'(j) = i} (x_i - y_j), j ascending: the entries of `sorted` equal
// to i, found by binary search; `order` names their j (a stable sort keeps them ascending).  fp64, rounded once.
__global__ __launch_bounds__(256) void chamfer_bwd_kernel(const float *__restrict__ x, const float *__restrict__ y, int P1, int P2,
                                                          const int32_t *__restrict__ nn, const int32_t *__restrict__ order,
                                                          const int32_t *__restrict__ sorted, double c_self, double c_other,
                                                          float *__restrict__ grad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P1) return;
    const double px = x[3 * (size_t)i], py = x[3 * (size_t)i + 1], pz = x[3 * (size_t)i + 2];
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (nn) {
        const int j = nn[i];
        if ((unsigned)j < (unsigned)P2) {
            gx = c_self * (px - (double)y[3 * (size_t)j]);
            gy = c_self * (py - (double)y[3 * (size_t)j + 1]);
            gz = c_self * (pz - (double)y[3 * (size_t)j + 2]);
        }
    }
    if (order) {
        int lo = 0, hi = P2;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sorted[mid] >= i) hi = mid; else lo = mid + 1;
        }
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int k = lo; k < P2 && sorted[k] == i; ++k) {
            const int j = order[k];
            if ((unsigned)j >= (unsigned)P2) continue;
            sx += px - (double)y[3 * (size_t)j]; sy += py - (double)y[3 * (size_t)j + 1]; sz += pz - (double)y[3 * (size_t)j + 2];
        }
        gx += c_other * sx; gy += c_other * sy; gz += c_other * sz;
    }
    grad[3 * (size_t)i] += (float)gx; grad[3 * (size_t)i + 1] += (float)gy; grad[3 * (size_t)i + 2] += (float)gz;
}

inline bool points_ok(int P) { return P >= 1 && P <= MAX_POINTS; }

}  // namespace

extern "C" int st3d_knn1_geometry(int P1, int P2, int *tile, int *segments) {
    ST3D_CHECK_ARG(tile && segments);
    ST3D_CHECK_ARG(points_ok(P1) && points_ok(P2));
    int seg_tiles;
    *segments = knn_segments(P1, P2, &seg_tiles);
    *tile = KNN_TILE;
    return ST3D_OK;
}

extern "C" size_t st3d_knn1_workspace_bytes(int P1, int P2) {
    if (!points_ok(P1) || !points_ok(P2)) return 0;
    int seg_tiles;
    return (size_t)knn_segments(P1, P2, &seg_tiles) * (size_t)P1 * 8;
}

extern "C" int st3d_knn1(const float *x, const float *y, int P1, int P2, void *workspace, size_t workspace_bytes, int32_t *idx,
                         float *dist, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && y && workspace && idx && dist);
    ST3D_CHECK_ARG(points_ok(P1) && points_ok(P2));
    ST3D_CHECK_ARG(workspace_bytes >= st3d_knn1_workspace_bytes(P1, P2) && ((uintptr_t)workspace & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    int seg_tiles;
    const int segments = knn_segments(P1, P2, &seg_tiles);
    float *seg_best = static_cast<float *>(workspace);
    int32_t *seg_idx = reinterpret_cast<int32_t *>(seg_best + (size_t)segments * P1);
    knn1_kernel<<<dim3(st3d::cdiv(P1, KNN_QBLOCK), segments), KNN_THREADS, 0, s>>>(x, y, P1, P2, seg_tiles, seg_best, seg_idx);
    ST3D_LAUNCH_CHECK();
    knn1_merge_kernel<<<st3d::cdiv(P1, 256), 256, 0, s>>>(x, y, P1, P2, segments, seg_best, seg_idx, idx, dist);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_face_area_cdf_scratch_bytes(int F) { return F >= 1 ? (size_t)st3d::cdiv(F, SCAN_BLOCK) * 8 : 0; }

extern "C" int st3d_face_area_cdf(const float *verts, const int32_t *faces, int F, void *scratch, size_t scratch_bytes, double *cdf,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && faces && scratch && cdf);
    ST3D_CHECK_ARG(F >= 1);
    ST3D_CHECK_ARG(scratch_bytes >= st3d_face_area_cdf_scratch_bytes(F) && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)cdf & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const int nb = st3d::cdiv(F, SCAN_BLOCK);
    double *totals = static_cast<double *>(scratch);
    area_scan_kernel<<<nb, SCAN_BLOCK, 0, s>>>(verts, faces, F, cdf, totals);
    ST3D_LAUNCH_CHECK();
    if (nb > 1) {
        totals_scan_kernel<<<1, SCAN_BLOCK, 0, s>>>(totals, nb);
        ST3D_LAUNCH_CHECK();
        cdf_offset_kernel<<<st3d::cdiv(F, 256), 256, 0, s>>>(cdf, totals, F);
        ST3D_LAUNCH_CHECK();
    }
    return ST3D_OK;
}

extern "C" int st3d_sample_points_fwd(const float *verts, const int32_t *faces, int F, const double *cdf, const float *r, int N,
                                      float *points, int32_t *face_idx, st3d_stream_t stream) {
    ST3D_CHECK_ARG(verts && faces && cdf && r && points && face_idx);
    ST3D_CHECK_ARG(F >= 1 && points_ok(N) && ((uintptr_t)cdf & 7) == 0);
    sample_fwd_kernel<<<st3d::cdiv(N, 256), 256, 0, st3d::as_stream(stream)>>>(verts, faces, F, cdf, r, N, points, face_idx);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_sample_points_bwd_scratch_bytes(int F) { return F >= 1 ? (size_t)F * 72 : 0; }

extern "C" int st3d_sample_points_bwd(const float *grad_points, const float *r, const int32_t *face_idx, int N, int F, int V,
                                      const int32_t *inc_off, const int32_t *inc_ref, void *scratch, size_t scratch_bytes,
                                      float *grad_verts, st3d_stream_t stream) {
    ST3D_CHECK_ARG(grad_points && r && face_idx && inc_off && inc_ref && scratch && grad_verts);
    ST3D_CHECK_ARG(F >= 1 && V >= 1 && points_ok(N));
    ST3D_CHECK_ARG(scratch_bytes >= st3d_sample_points_bwd_scratch_bytes(F) && ((uintptr_t)scratch & 7) == 0);
    hipStream_t s = st3d::as_stream(stream);
    double *blocks = static_cast<double *>(scratch);
    sample_bwd_face_kernel<<<st3d::cdiv(F, 256), 256, 0, s>>>(grad_points, r, face_idx, N, F, blocks);
    ST3D_LAUNCH_CHECK();
    sample_bwd_vertex_kernel<<<st3d::cdiv(V, 256), 256, 0, s>>>(blocks, inc_off, inc_ref, V, F, grad_verts);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_chamfer_sum(const float *dist, int P, double scale, float *loss, st3d_stream_t stream) {
    ST3D_CHECK_ARG(dist && loss);
    ST3D_CHECK_ARG(points_ok(P));
    chamfer_sum_kernel<<<1, SCAN_BLOCK, 0, st3d::as_stream(stream)>>>(dist, P, scale, loss);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_chamfer_bwd(const float *x, const float *y, int P1, int P2, const int32_t *nn, const int32_t *order,
                                const int32_t *sorted, double c_self, double c_other, float *grad_x, st3d_stream_t stream) {
    ST3D_CHECK_ARG(x && y && grad_x);
    ST3D_CHECK_ARG(points_ok(P1) && points_ok(P2));
    ST3D_CHECK_ARG((nn || order) && (order == nullptr) == (sorted == nullptr));
    chamfer_bwd_kernel<<<st3d::cdiv(P1, 256), 256, 0, st3d::as_stream(stream)>>>(x, y, P1, P2, nn, order, sorted, c_self, c_other,
                                                                                grad_x);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
