// diffuse.hip -- Laplacian-preconditioned vertex steps (Nicolet, Jacobson, Jakob, "Large Steps in Inverse Rendering of
// Geometry", 2021): the matrix M = I + lambda L of the mesh's static topology, L the combinatorial Laplacian
//     (L x)_i = sum over j in nbr(i), in adjacency order, of (x_i - x_j)
// applied (st3d_diffuse_apply) and inverted by plain conjugate gradients (st3d_diffuse_solve), and the Adam update with one
// second-moment denominator for the whole tensor that the paper runs on u = M v (st3d_adam_step_uniform).
//
// The row is accumulated as differences, never as deg_i x_i - sum x_j: a constant vector is then annihilated exactly, so
// M c = c bit for bit and a constant right-hand side is solved in one iteration with alpha = 1.  The file is built with
// -ffp-contract=off: every rounding is the one written here.
//
// The solve: three workgroups of 1024 threads, one per coordinate column; the columns are independent systems.  The whole
// iteration loop runs inside the kernel and a workgroup synchronises with __syncthreads() alone -- there is no barrier,
// flag or wait between workgroups anywhere, so the launch makes progress whether or not its three workgroups are resident
// together.  Thread t owns rows t, t + 1024, ...: x, r and A p are read and written by their owner only -- in registers
// while a thread owns at most four rows (V <= 4096), else in the output and the workspace; the search direction p is the
// one vector read across threads, and lives in LDS while 4 V + 256 bytes fit the 160 KiB a gfx950 workgroup may take, else
// in the workspace.  Every home sees the same arithmetic in the same order.  Dot products: fp32 products, added in fp64 serially over a thread's rows, then down a fixed shuffle tree of the
// wave and a fixed tree over the 16 waves that every thread evaluates itself from LDS -- alpha, beta and the decision to
// stop are therefore the same bits in every thread and every barrier sits in uniform control flow.  No atomics.
// The loop is bounded by max_iter and nothing else: a NaN makes every comparison false and the loop runs to max_iter.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int NT = 1024;                    // threads of a solver workgroup
constexpr int NW = NT / 64;                 // its waves
constexpr size_t RED_BYTES = 2 * NW * sizeof(double);      // two reduction scratch arrays in front of p in LDS
constexpr size_t LDS_LIMIT = 160 * 1024;    // what one workgroup may take on gfx950
constexpr size_t LDS_DEFAULT = 64 * 1024;   // above this the dynamic size is an opt-in per kernel
constexpr int REG_ROWS = 4;                 // up to this many rows per thread (V <= 4096) x, r and A p stay in registers

__host__ __device__ inline size_t padded(int V) { return ((size_t)V + 3) & ~(size_t)3; }

__device__ __forceinline__ float row_apply(const int *__restrict__ nbr_off, const int *__restrict__ nbr_idx, int i,
                                           float lambda, float xi, const float *x, int stride) {
    float l = 0.f;
    const int e1 = nbr_off[i + 1];
    for (int e = nbr_off[i]; e < e1; ++e) l += xi - x[(size_t)nbr_idx[e] * stride];
    return xi + lambda * l;
}

__global__ __launch_bounds__(256) void apply_kernel(const int *__restrict__ nbr_off, const int *__restrict__ nbr_idx, int V,
                                                    float lambda, const float *__restrict__ x, float *__restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    for (int c = 0; c < 3; ++c) y[(size_t)3 * i + c] = row_apply(nbr_off, nbr_idx, i, lambda, x[(size_t)3 * i + c], x + c, 3);
}

// sum of v over the workgroup, the same bits in every thread.  `red` (NW doubles of LDS) must not be written again before
// another barrier has passed: the callers alternate between two arrays.
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) s[w] = red[w];
#pragma unroll
    for (int n = NW / 2; n > 0; n >>= 1)
#pragma unroll
        for (int w = 0; w < n; ++w) s[w] = s[2 * w] + s[2 * w + 1];
    return s[0];
}

struct SolveInfo { int iterations, converged; float residual; };

// RPT > 0: V <= RPT * NT, and x, r and A p of a thread's (at most RPT) rows stay in registers for the whole solve -- the
// workspace is not touched and an iteration waits on LDS alone.  RPT == 0: they live in the output and the workspace.
// ROWS(k, i): the thread's rows i = t + k NT; with RPT > 0 the loop unrolls fully (NR = RPT) and k indexes the registers
// statically; with RPT == 0 it stays a loop (NR = 1).
#define ROWS(k, i) _Pragma("unroll NR") for (int k = 0, i = t; (RPT == 0 || k < RPT) && i < V; ++k, i += NT)

template <bool P_IN_LDS, int RPT>
__global__ __launch_bounds__(NT) void solve_kernel(const int *__restrict__ nbr_off, const int *__restrict__ nbr_idx, int V,
                                                   float lambda, const float *__restrict__ b, float *__restrict__ x,
                                                   double tol2, int max_iter, float *ws, SolveInfo *info) {
    static_assert(RPT == 0 || P_IN_LDS, "the register variant is for meshes whose search direction fits LDS");
    extern __shared__ double lds[];
    double *red0 = lds, *red1 = lds + NW;
    const int c = blockIdx.x, t = threadIdx.x;
    const size_t Vp = padded(V);
    float *r = ws + (size_t)c * 3 * Vp, *Ap = r + Vp;
    float *p = P_IN_LDS ? reinterpret_cast<float *>(lds + 2 * NW) : Ap + Vp;
    const float *bc = b + c;
    float *xc = x + c;
    constexpr int NR = RPT > 0 ? RPT : 1;
    float xr[NR], rg[NR], ag[NR];

    double acc = 0.0;
    ROWS(k, i) {
        const float bi = bc[(size_t)3 * i];
        if constexpr (RPT > 0) { xr[k] = 0.f; rg[k] = bi; } else { xc[(size_t)3 * i] = 0.f; r[i] = bi; }
        p[i] = bi;
        acc += (double)(bi * bi);
    }
    const double bb = block_sum(acc, red0);          // its barrier also publishes p
    double rr = bb;
    int it = 0, converged = 0;
    if (bb == 0.0) {                                 // b = 0: x = 0 after 0 iterations, no division (a NaN is not == 0)
        converged = 1;
    } else {
        const double stop = tol2 * bb;
        while (it < max_iter) {
            acc = 0.0;
            ROWS(k, i) {
                const float pi = p[i];
                const float a = row_apply(nbr_off, nbr_idx, i, lambda, pi, p, 1);
                if constexpr (RPT > 0) ag[k] = a; else Ap[i] = a;
                acc += (double)(pi * a);
            }
            const float alpha = (float)(rr / block_sum(acc, red1));
            acc = 0.0;
            ROWS(k, i) {
                float ri;
                if constexpr (RPT > 0) {
                    xr[k] = xr[k] + alpha * p[i];
                    ri = rg[k] - alpha * ag[k];
                    rg[k] = ri;
                } else {
                    xc[(size_t)3 * i] = xc[(size_t)3 * i] + alpha * p[i];
                    ri = r[i] - alpha * Ap[i];
                    r[i] = ri;
                }
                acc += (double)(ri * ri);
            }
            const double rr_new = block_sum(acc, red0);
            ++it;
            if (rr_new <= stop) { rr = rr_new; converged = 1; break; }       // uniform: rr_new is the same bits everywhere
            const float beta = (float)(rr_new / rr);
            rr = rr_new;
            ROWS(k, i) {
                float ri;
                if constexpr (RPT > 0) ri = rg[k]; else ri = r[i];
                p[i] = ri + beta * p[i];
            }
            __syncthreads();                          // every p_i is written before any row reads it
        }
    }
    if constexpr (RPT > 0) {
        ROWS(k, i) xc[(size_t)3 * i] = xr[k];
    }
    if (t == 0) {
        info[c].iterations = it;
        info[c].converged = converged;
        info[c].residual = bb == 0.0 ? 0.f : (float)sqrt(rr / bb);
    }
}
#undef ROWS

// ---- Adam with one denominator for the whole tensor
constexpr int NPART = 1024;

// the larger of the two, a NaN if either is one (it then reaches every parameter); free of the order it is applied in
__device__ __forceinline__ float nan_max(float a, float b) { return b > a || b != b ? b : a; }

__global__ __launch_bounds__(256) void adam_uniform_moments_kernel(const float *__restrict__ g, float *__restrict__ m,
                                                                   float *__restrict__ v, size_t n, float b1, float b2,
                                                                   float *__restrict__ partials) {
    __shared__ float s[4];
    float hi = 0.f;                                  // second moments are >= 0
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        m[i] = m[i] + (gi - m[i]) * (1.0f - b1);
        const float vi = v[i] * b2 + (1.0f - b2) * gi * gi;
        v[i] = vi;
        hi = nan_max(hi, vi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        hi = nan_max(hi, __shfl_down(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = hi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) hi = nan_max(hi, s[w]);
        partials[blockIdx.x] = hi;
    }
}

__global__ __launch_bounds__(256) void adam_uniform_update_kernel(float *__restrict__ p, const float *__restrict__ m, size_t n,
                                                                  float lr, float bc1, float bc2, float eps,
                                                                  const float *__restrict__ partials, int np) {
    __shared__ float s[256];
    float hi = 0.f;
    for (int i = threadIdx.x; i < np; i += 256) {
        hi = nan_max(hi, partials[i]);
    }
    s[threadIdx.x] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = nan_max(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    const float denom = eps + sqrtf(s[0] / bc2);     // max over all of sqrt(v / bc2): the square root is monotone
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        p[i] = p[i] - lr * ((m[i] / bc1) / denom);
}

inline int grid_for(size_t n) {
    const size_t blocks = (n + 255) / 256;
    return (int)(blocks < (size_t)NPART ? blocks : (size_t)NPART);
}

// ST3D_DIFFUSE_LDS=0: the search direction in the workspace whatever V is; ST3D_DIFFUSE_REGS=0: x, r and A p in the output
// and the workspace whatever V is.  Both are read by every call (A/B runs, tests); every combination gives the same bits.
bool env_on(const char *name) {
    const char *e = getenv(name);
    return !(e && e[0] == '0' && e[1] == 0);
}

bool topology_ok(const int *nbr_off, const int *nbr_idx, int V) { return nbr_off && nbr_idx && V >= 1; }

}  // namespace

extern "C" int st3d_diffuse_apply(const int *nbr_off, const int *nbr_idx, int V, float lambda, const float *x, float *y,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(topology_ok(nbr_off, nbr_idx, V) && x && y && x != y);
    ST3D_CHECK_ARG(isfinite(lambda) && lambda >= 0.f);
    apply_kernel<<<st3d::cdiv(V, 256), 256, 0, st3d::as_stream(stream)>>>(nbr_off, nbr_idx, V, lambda, x, y);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" size_t st3d_diffuse_workspace_bytes(int V) {
    return V >= 1 ? (size_t)9 * padded(V) * sizeof(float) : 0;
}

extern "C" int st3d_diffuse_solve(const int *nbr_off, const int *nbr_idx, int V, float lambda, const float *b, float *x,
                                  float tol, int max_iter, void *workspace, size_t workspace_bytes, void *info,
                                  st3d_stream_t stream) {
    ST3D_CHECK_ARG(topology_ok(nbr_off, nbr_idx, V) && b && x && b != x && info);
    ST3D_CHECK_ARG(isfinite(lambda) && lambda >= 0.f);
    ST3D_CHECK_ARG(tol > 0.f && isfinite(tol));
    ST3D_CHECK_ARG(max_iter >= 1);
    ST3D_CHECK_ARG(workspace && workspace_bytes >= st3d_diffuse_workspace_bytes(V));
    ST3D_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)info & 3) == 0);
    hipStream_t s = st3d::as_stream(stream);
    const double tol2 = (double)tol * (double)tol;
    const size_t with_p = RED_BYTES + (size_t)V * sizeof(float);
    const bool in_lds = env_on("ST3D_DIFFUSE_LDS") && with_p <= LDS_LIMIT;
    float *ws = (float *)workspace;
    SolveInfo *out = (SolveInfo *)info;
    if (in_lds && V <= REG_ROWS * NT && env_on("ST3D_DIFFUSE_REGS")) {       // with_p <= 256 + 16 KiB: no opt-in needed
        solve_kernel<true, REG_ROWS><<<3, NT, with_p, s>>>(nbr_off, nbr_idx, V, lambda, b, x, tol2, max_iter, ws, out);
    } else if (in_lds) {
        if (with_p > LDS_DEFAULT)       // an attribute of this instantiation on the current device; set whenever it is needed
            ST3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(solve_kernel<true, 0>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)with_p));
        solve_kernel<true, 0><<<3, NT, with_p, s>>>(nbr_off, nbr_idx, V, lambda, b, x, tol2, max_iter, ws, out);
    } else {
        solve_kernel<false, 0><<<3, NT, RED_BYTES, s>>>(nbr_off, nbr_idx, V, lambda, b, x, tol2, max_iter, ws, out);
    }
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}

extern "C" int st3d_adam_step_uniform(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step,
                                      float lr, float beta1, float beta2, float eps, float *partials, st3d_stream_t stream) {
    ST3D_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && partials);
    ST3D_CHECK_ARG(n > 0 && step >= 1);
    hipStream_t s = st3d::as_stream(stream);
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2 = (float)(1.0 - pow((double)beta2, (double)step));
    const int gsz = grid_for(n);
    adam_uniform_moments_kernel<<<gsz, 256, 0, s>>>(grad, exp_avg, exp_avg_sq, n, beta1, beta2, partials);
    ST3D_LAUNCH_CHECK();
    adam_uniform_update_kernel<<<gsz, 256, 0, s>>>(param, exp_avg, n, lr, bc1, bc2, eps, partials, gsz);
    ST3D_LAUNCH_CHECK();
    return ST3D_OK;
}
