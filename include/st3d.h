/*
 * st3d.h -- C ABI of libst3d.so: the MI355X (gfx950) device half of the 2D->3D
 * style-transfer optimisation step.
 *
 * The reference (EmaMule/2D-to-3D-Style-Transfer) is pure Python and has no FFI of its
 * own: what it binds for this path is PyTorch3D's `_C` extension, torchvision/ATen
 * operators and torch.optim.Adam.  Each entry point below cites the reference call site
 * (file:line, relative to the reference tree) whose device work it replaces.
 *
 * Conventions
 *   - extern "C"; plain pointers and sizes; no torch / C++ types.
 *   - every pointer is a DEVICE pointer owned by the caller unless it is marked `host`;
 *     opaque handles (st3d_vgg, st3d_plan) own their workspaces (hipMalloc at create).
 *   - every function returns 0 (ST3D_OK) or a negative ST3D_E_* code; st3d_last_error()
 *     returns a thread-local message.  No exceptions cross the boundary.
 *   - kernels are asynchronous on the given stream (a hipStream_t passed as void*; NULL =
 *     the default stream).  Handles are not thread-safe (the reference is single-threaded).
 *   - tensors are fp32, contiguous; images are NCHW exactly as utils.py:70-76 builds them.
 *
 * Run-time switches the shipped library reads from the environment.  The defaults are the
 * measured-best paths; every other value exists for same-box A/B runs and gives the same
 * results (to fp32 summation order where a split count changes).
 *   ST3D_CONV=direct            direct implicit-GEMM convolutions (conv.hip) instead of Winograd
 *   ST3D_WINO43=0, ST3D_WINO43_MINK=k   never run the F(4x4,3x3) Winograd kernel (wino43.hip) / only from k input channels (default 64)
 *   ST3D_W43_SLOTS=n            persistent workgroups per cout tile of the F(4x4,3x3) kernel (default: CUs / cout tiles)
 *   ST3D_W43_XCD=0              its slots in tile order instead of XCD-major
 *   ST3D_WINO_MAP=rr|xcd        block -> tile mapping of the F(2x2,3x3) Winograd launches
 *   ST3D_PREGATE=0              every input-gradient applies its own ReLU gate (consumer side)
 *   ST3D_TAP0_FUSED=0, ST3D_TAP0_J=1   separate relu1_1 Gram backward + conv1_1 input gradient / 4-byte accesses
 *   ST3D_GRAM_MULTI=0           the five Gram forwards as separate launches (st3d_gram_fwd_multi)
 *   ST3D_GRAM_MULTI_SCALE=n, ST3D_GRAM_MULTI_SCALES=a,b,c,d, ST3D_GRAM_MULTI_DEAL=1   split-K width / block order of the fused launch
 *   ST3D_GRAM_FAST=0, ST3D_GRAM_DIAG_TRI=0, ST3D_GRAM_TARGET_WGS, ST3D_GRAM_NSPLIT   Gram forward: generic / full-tile kernels, split counts
 *   ST3D_GRAM_BWD_MT, ST3D_GRAM_BWD_K64, ST3D_GRAM_BWD_SYM=0   Gram backward tile shapes / the general kernel
 *   ST3D_RASTER_BINS=0          flat face sweep instead of the coarse 64x64-pixel bins
 *   ST3D_RASTER_WALK=1          hard rasteriser: every pixel walks its tile's face list instead of faces in parallel per tile (read per call)
 *   ST3D_POISON_PLAN=1          plan workspaces start as 0xFF (read-before-write detector of the tests)
 *   ST3D_ROCTX=1                roctx ranges around the phases of a step (st3d_trace_push / st3d_trace_pop below)
 * Read by the Python host (st3d/): ST3D_DETERMINISTIC=0 (float-atomic scatters), ST3D_GRAPH=1 (HIP-graph replay of
 * the loss step), ST3D_NEAR_PLANE=raise, ST3D_MAX_PLANS, ST3D_VGG19_WEIGHTS, ST3D_DIST_BACKEND, ST3D_NCCL.
 * Lab builds only (ST3D_LAB=1 python build.py; never shipped): ST3D_WINO_VARIANT=8 (the retired 8-wave Winograd
 * kernel, csrc/lab/wino8.inc), ST3D_WINO_DBGMODE / ST3D_WINO_STAMP (diagnostic instantiations, s_memtime stamps).
 */
#ifndef ST3D_H
#define ST3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST3D_OK 0
#define ST3D_E_INVALID (-1) /* bad argument / shape */
#define ST3D_E_HIP (-2)     /* a HIP runtime call failed */
#define ST3D_E_NOMEM (-3)   /* workspace allocation failed */
#define ST3D_E_STATE (-4)   /* call order violated (e.g. loss before targets) */

typedef void *st3d_stream_t;

int st3d_version(void);
const char *st3d_last_error(void);
/* host out-params; any may be NULL */
int st3d_device_info(int device, int *cu_count, size_t *hbm_bytes, char *name, int name_len);

/* ------------------------------------------------------------------ render: utils.py:65-77
 * (render_meshes -> PyTorch3D MeshRasterizer/SoftPhongShader configured at
 *  first_approach.py:107-113, second_approach.py:101-108: blur_radius=0, faces_per_pixel=1,
 *  ambient lights, FoV perspective cameras).  All B views of a batch go through one launch. */

/* verts (V,3) world; R (B,3,3), T (B,3) row-vector convention X_view = X R + T
 * (utils.py:142-149,161-168); out verts_ndc (B,V,3) = (x_ndc, y_ndc, z_view). */
int st3d_project_verts(const float *verts, int V, const float *R, const float *T, int B,
                       float inv_tan_half_fov, float *verts_ndc, st3d_stream_t stream);

/* bytes of scratch st3d_raster_fwd needs: per-view face records (48 B per face) + packed tile ranges (4 B per face) */
size_t st3d_raster_workspace_bytes(int B, int F);
/* the same + room for the coarse face bins of st3d_raster_fwd (lists of the faces touching each 64 x 64-pixel bin, built
 * per call): with a workspace of this size a tile sweeps its bin's list instead of every face (meshes of more than 2048
 * faces); with the smaller one st3d_raster_fwd keeps the flat sweep.  Same results either way. */
size_t st3d_raster_workspace_bytes_binned(int B, int F, int S);

/* Hard rasterisation (K=1, blur_radius=0, perspective-correct barycentrics).
 * faces (F,3) int32.  Outputs per view (B,S,S): pix_to_face int32 (-1 = background; the
 * reference's int64 is produced by the Python host on request), zbuf, bary (B,S,S,3),
 * dists (signed squared edge distance), -1 filled on background. */
int st3d_raster_fwd(const float *verts_ndc, const int32_t *faces, int B, int V, int F, int S,
                    void *workspace, size_t workspace_bytes, int32_t *pix_to_face, float *zbuf,
                    float *bary, float *dists,
                    float z_clip, int32_t *near_flag /* device int, may be NULL: OR-ed with 1 when a rasterised face has a
                    vertex nearer than z_clip -- PyTorch3D would clip it (znear / 2); this K = 1 path does not, use the
                    general kernels (st3d_face_setup_clip) then */,
                    st3d_stream_t stream);

/* Fused TexturesUV.sample_textures + ambient shading + softmax_rgb_blend (K=1) + the
 * RGB/mask extraction of utils.py:70-72.  texture (T,T,3) HWC as maps_padded()[0]
 * (utils.py:208), verts_uvs (VT,2), faces_uvs (F,3) int32.
 * rgb (B,3,S,S), mask (B,1,S,S) = (alpha > 0). */
int st3d_shade_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf,
                   const float *dists, const float *verts_uvs, const int32_t *faces_uvs,
                   const float *texture, int B, int S, int T, int F, int VT, float *rgb,
                   float *mask, st3d_stream_t stream);

/* Texture-sampling backward (grid_sampler_2d_backward + blend backward):
 * grad_rgb (B,3,S,S) -> grad_texture (T,T,3), ACCUMULATED over the B views (caller zeroes).
 * Optional outputs for the vertex path (NULL for texture-only optimisation): grad_uv (B,S,S,2)
 * = d loss / d (u,v) and grad_bary (B,S,S,3) = d loss / d barycentrics (interpolate_face_attributes
 * backward).  grad_texture may be NULL when only the vertices are optimised. */
int st3d_shade_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary,
                   const float *zbuf, const float *dists, const float *verts_uvs,
                   const int32_t *faces_uvs, const float *texture, int B, int S, int T, int F,
                   int VT, float *grad_texture, float *grad_uv, float *grad_bary,
                   st3d_stream_t stream);

/* Rasteriser backward (PyTorch3D RasterizeMeshesBackward, grad_bary path; reached through
 * loss.backward() at second_approach.py:188 when optimization_target is 'mesh'/'both'):
 * grad_bary (B,S,S,3) -> grad_verts_ndc (B,V,3) (zeroed by the call, then atomically summed). */
int st3d_raster_bwd(const float *grad_bary, const int32_t *pix_to_face, const float *verts_ndc,
                    const int32_t *faces, int B, int V, int F, int S, float *grad_verts_ndc,
                    st3d_stream_t stream);
/* backward of st3d_project_verts: grad_verts (V,3) (+)= sum over the B views */
int st3d_project_verts_bwd(const float *verts, int V, const float *R, const float *T, int B,
                           float inv_tan_half_fov, const float *grad_verts_ndc, int accumulate,
                           float *grad_verts, st3d_stream_t stream);

/* ---- bitwise reproducible variants of the two gradient scatters ("deterministic variant").
 * The default kernels sum with float atomics, so the last bits of the texture / vertex gradient depend on the order
 * the hardware serves them; these accumulate in 64-bit fixed point with a power-of-two scale taken from a bound on the
 * partial sums (integer addition is associative: any order gives the same bits), then convert.  Same arguments and
 * results (to fp32 rounding of the final sums) as st3d_shade_bwd / st3d_raster_bwd, plus a caller-owned workspace. */
size_t st3d_shade_bwd_det_workspace_bytes(int T);
int st3d_shade_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                       const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                       int B, int S, int T, int F, int VT, float *grad_texture /* accumulated into */, float *grad_uv,
                       float *grad_bary, void *workspace, size_t workspace_bytes, st3d_stream_t stream);
size_t st3d_raster_bwd_det_workspace_bytes(int B, int V, int S);
int st3d_raster_bwd_det(const float *grad_bary, const int32_t *pix_to_face, const float *verts_ndc, const int32_t *faces,
                        int B, int V, int F, int S, float *grad_verts_ndc, void *workspace, size_t workspace_bytes,
                        st3d_stream_t stream);

/* ---- general soft renderer: PyTorch3D's MeshRasterizer / SoftPhongShader under any other
 * RasterizationSettings / BlendParams than the ones the reference constructs at first_approach.py:107-113 and
 * second_approach.py:101-108 (K = 1, blur_radius = 0, default blend, served by the entry points above):
 * K = faces_per_pixel <= 8 nearest faces per pixel, blur_radius >= 0, barycentric clipping (PyTorch3D clips when
 * blur_radius > 0), cull_backfaces, perspective_correct on/off, softmax_rgb_blend over the K layers with sigma / gamma / background (host float[3]).
 * Fragment arrays are (B,S,S,K[,3]), depth-sorted, -1 filled. */
int st3d_face_setup(const float *verts_ndc, const int32_t *faces, int B, int V, int F, void *face_records,
                    size_t records_bytes /* >= st3d_raster_workspace_bytes */, st3d_stream_t stream);
/* Near-plane clipping (PyTorch3D clips against z = z_clip_value = znear / 2 for perspective cameras before rasterising):
 * two record slots per face -- the face itself or its part in front of the plane as one or two triangles
 * (B * 2F records, st3d_clip_records_bytes); st3d_raster_soft_fwd then runs with records_per_face = 2, reports the ORIGINAL
 * face in pix_to_face, converts the barycentrics back to it and writes the record slot of every fragment to frag_slot
 * (B,S,S,K), which st3d_raster_soft_bwd needs to differentiate through the clip. */
size_t st3d_clip_records_bytes(int B, int F);
int st3d_face_setup_clip(const float *verts_ndc, const int32_t *faces, int B, int V, int F, float z_clip,
                         int perspective_correct, void *face_records, size_t records_bytes, st3d_stream_t stream);
int st3d_raster_soft_fwd(const float *face_records, int B, int F, int S, int K, float blur_radius, int clip_bary,
                         int cull_backfaces /* skip faces whose NDC area is negative */,
                         int perspective_correct /* 0: screen-space barycentrics */,
                         int records_per_face /* 1: st3d_face_setup records; 2: st3d_face_setup_clip records */,
                         int32_t *frag_slot /* (B,S,S,K) or NULL */,
                         int32_t *pix_to_face, float *zbuf, float *bary, float *dists, st3d_stream_t stream);
int st3d_shade_soft_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                        const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int T,
                        int K, float sigma, float gamma, const float *background, float *rgb, float *alpha,
                        st3d_stream_t stream);
/* grad_rgb (B,3,S,S) -> grad_texture (T,T,3) accumulated, per-layer grad_bary (B,S,S,K,3), grad_zbuf, grad_dists
 * (B,S,S,K); any output may be NULL */
int st3d_shade_soft_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                        const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                        int B, int S, int T, int K, float sigma, float gamma, const float *background,
                        float *grad_texture, float *grad_bary, float *grad_zbuf, float *grad_dists,
                        st3d_stream_t stream);
/* PyTorch3D RasterizeMeshesBackward: (grad_bary, grad_zbuf, grad_dists) -> grad_verts_ndc (B,V,3), zeroed by the call */
int st3d_raster_soft_bwd(const float *grad_bary, const float *grad_zbuf, const float *grad_dists,
                         const int32_t *pix_to_face, const float *verts_ndc, const int32_t *faces, int B, int V, int F,
                         int S, int K, int clip_bary, int perspective_correct,
                         const int32_t *frag_slot /* from the clipped forward, or NULL */, float z_clip,
                         float *grad_verts_ndc, st3d_stream_t stream);
/* The two scatters above with bitwise reproducible results: the same per-tile LDS binning (per texel / per face) in
 * 64-bit fixed point (csrc/det.h), like st3d_shade_bwd_det / st3d_raster_bwd_det for the specialised K = 1 path.
 * grad_texture must be given (it is accumulated into); workspace 16-byte aligned.  A non-finite input gradient gives a
 * NaN result (never a laundered finite one). */
size_t st3d_shade_soft_bwd_det_workspace_bytes(int T);
int st3d_shade_soft_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                            const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                            int B, int S, int T, int K, float sigma, float gamma, const float *background,
                            float *grad_texture, float *grad_bary, float *grad_zbuf, float *grad_dists,
                            void *workspace, size_t workspace_bytes, st3d_stream_t stream);
size_t st3d_raster_soft_bwd_det_workspace_bytes(int B, int V, int S);
int st3d_raster_soft_bwd_det(const float *grad_bary, const float *grad_zbuf, const float *grad_dists,
                             const int32_t *pix_to_face, const float *verts_ndc, const int32_t *faces, int B, int V, int F,
                             int S, int K, int clip_bary, int perspective_correct, const int32_t *frag_slot, float z_clip,
                             float *grad_verts_ndc, void *workspace, size_t workspace_bytes, st3d_stream_t stream);

/* ---- silhouette (csrc/silhouette.hip): PyTorch3D's SoftSilhouetteShader on the fragments of st3d_raster_soft_fwd.  The
 * reference never builds one (it only thresholds alpha, utils.py:72); this is the image-space anchor PyTorch3D offers
 * for the runs that move the mesh.  Over the K <= 8 layers of a pixel, skipping pix_to_face_k < 0:
 *   prob_k = sigmoid(-dists_k / sigma),  alpha = 1 - prod_k (1 - prob_k),
 *   d alpha / d dists_k = -prob_k * prod_j (1 - prob_j) / sigma.
 * alpha equals st3d_shade_soft_fwd's bit for bit.  pix_to_face, dists, grad_dists are (B,S,S,K); alpha, grad_alpha and
 * target are (B,1,S,S); sigma > 0. */
/* pytorch3d.renderer.blending.sigmoid_alpha_blend(colors, fragments, blend_params)[..., 3] (SoftSilhouetteShader.forward) */
int st3d_silhouette_fwd(const int32_t *pix_to_face, const float *dists, int B, int S, int K, float sigma, float *alpha,
                        st3d_stream_t stream);
/* autograd's backward of sigmoid_alpha_blend for its alpha channel: grad_dists = (accumulate ? grad_dists : 0) +
 * grad_alpha * d alpha / d dists; empty layers get 0 (accumulate: are left alone) */
int st3d_silhouette_bwd(const float *grad_alpha, const int32_t *pix_to_face, const float *dists, int B, int S, int K,
                        float sigma, int accumulate, float *grad_dists, st3d_stream_t stream);
/* ((sigmoid_alpha_blend(...)[..., 3] - target) ** 2).sum() * scale and its backward to dists in one pass (neither alpha nor
 * its gradient goes to memory): loss_out[0] += scale * sum (alpha - target)^2 by the ordered two-stage reduction (partials:
 * st3d_reduce_partials() floats; bitwise reproducible), grad_dists (may be NULL) = 2 * scale * (alpha - target) *
 * d alpha / d dists -- bit for bit what st3d_silhouette_bwd gives for grad_alpha = 2 * scale * (st3d_silhouette_fwd - target).
 * scale carries the weight, 1 / S^2 and the GLOBAL batch denominator. */
int st3d_silhouette_loss(const int32_t *pix_to_face, const float *dists, const float *target, int B, int S, int K,
                         float sigma, float scale, float *grad_dists, float *partials, float *loss_out,
                         st3d_stream_t stream);

/* ---- silhouette rasteriser (csrc/silraster.hip): SoftSilhouetteShader at faces_per_pixel K = 1..64 without fragments in
 * memory.  face_records are st3d_face_setup_clip's (two per face, st3d_clip_records_bytes).  Per pixel: the candidates are
 * the records that pass ref_rasterize_k3's tests (oracle/raster_ref.c), of a quadrilateral split by the near plane the half
 * nearer in the image plane counts, the K nearest by (depth, record index) are the fragments, and
 *   prob_k = sigmoid(-d_k / sigma),  keep = prod_k (1 - prob_k) in depth order,  alpha = 1 - keep
 * -- at K <= 8 bit for bit st3d_silhouette_fwd on st3d_raster_soft_fwd's fragments.  `state` is what the backward needs,
 * planes of B*S*S floats: keep, the depth and the record index (int bits) of the last fragment taken, and for the fused
 * loss alpha - target: 12 / 16 bytes per pixel whatever K is.  alpha and target are (B,1,S,S); sigma > 0;
 * blur_radius >= 0.  A candidate with a NaN depth or distance makes its pixel's keep, alpha and gradient NaN. */
/* rasterize_meshes(faces_per_pixel=K, blur_radius, clip_barycentric_coords, cull_backfaces, perspective_correct, z_clip_value)
 * + blending.sigmoid_alpha_blend(...)[..., 3]; state: 3 planes */
int st3d_silraster_fwd(const float *face_records, int B, int F, int S, int K, float blur_radius, int clip_bary,
                       int cull_backfaces, int perspective_correct, float sigma, float *alpha, float *state,
                       st3d_stream_t stream);
/* the same followed by ((alpha - target) ** 2).sum() * scale: loss_out[0] += that, by st3d_silhouette_loss's ordered
 * reduction (partials: st3d_reduce_partials() floats; bitwise reproducible, and bit for bit st3d_silhouette_loss's value
 * where alpha is).  alpha does not reach memory; state: 4 planes */
int st3d_silraster_loss(const float *face_records, int B, int F, int S, int K, float blur_radius, int clip_bary,
                        int cull_backfaces, int perspective_correct, float sigma, const float *target, float scale, float *state,
                        float *partials, float *loss_out, st3d_stream_t stream);
/* autograd's backward of the two above down to the projected vertices (rasterize_meshes' backward for dists +
 * sigmoid_alpha_blend's): grad_verts_ndc (B,V,3) = sum over the fragments of upstream * (-prob * keep / sigma) * d d / d verts
 * (nearest edge, first minimum, projection parameter constant; through the cut points on clipped faces, z_clip as given to
 * st3d_face_setup_clip).  upstream = grad_alpha (B,1,S,S), or with grad_alpha NULL grad_scale * (plane 3 of the fused loss's
 * state), grad_scale = 2 * scale.  workspace (st3d_silraster_bwd_workspace_bytes, 16-byte aligned): 64-bit fixed-point
 * accumulation after a bound pass, bitwise reproducible; NULL: float atomics.  No gradient to cameras. */
size_t st3d_silraster_bwd_workspace_bytes(int B, int V, int S);
int st3d_silraster_bwd(const float *face_records, const float *verts_ndc, const int32_t *faces, int B, int V, int F, int S,
                       float blur_radius, int clip_bary, int cull_backfaces, int perspective_correct, float z_clip, float sigma,
                       const float *state, const float *grad_alpha, float grad_scale, float *grad_verts_ndc, void *workspace,
                       size_t workspace_bytes, st3d_stream_t stream);

/* ---- Phong lighting (PyTorch3D SoftPhongShader with PointLights / DirectionalLights / AmbientLights and Materials;
 * csrc/phong.h holds the per-fragment formulas, csrc/lighting.hip the mesh side).  World space throughout: vertex normals
 * n_v = m_v / max(|m_v|, 1e-6), m_v = sum over v's faces of (v2 - v1) x (v0 - v1); per fragment N = sum b_i n_i,
 * P = sum b_i v_i, camera centre C = -T R^T (from R, T of the view); colour = (A + D) * texel + Sp replaces the texel in
 * the blend (no clamping; the background is not lit).
 *
 * Light block: n_lights (1, or B = one per view) entries of 24 floats:
 *   [0..2] ambient_color  [3..5] diffuse_color  [6..8] specular_color  [9..11] location (point) / direction (directional)
 *   [12..14] material ambient  [15..17] material diffuse  [18..20] material specular  [21] shininess  [22..23] unused
 * kind: 0 ambient only (colour = ka La texel; verts / normals may be NULL), 1 point, 2 directional, 3 point light at each
 * view's camera centre (headlight; [9..11] unused).
 *
 * Incidence list of the vertex normals: inc_off (V+1), inc_ref (3F) = face * 3 + corner, ascending within each vertex. */
size_t st3d_vertex_normals_scratch_floats(int F);
/* normals (V,3) and the unnormalised sums m (V,3) the backward needs; scratch >= st3d_vertex_normals_scratch_floats */
int st3d_vertex_normals(const float *verts, const int32_t *faces, int V, int F, const int32_t *inc_off,
                        const int32_t *inc_ref, float *scratch, float *normals, float *unnormalised, st3d_stream_t stream);
/* grad_verts (V,3) += grad_pos (may be NULL) + d/dverts of <grad_normals, normals(verts)> */
int st3d_vertex_normals_bwd(const float *verts, const int32_t *faces, int V, int F, const int32_t *inc_off,
                            const int32_t *inc_ref, const float *unnormalised, const float *grad_normals,
                            const float *grad_pos, float *scratch, float *grad_verts, st3d_stream_t stream);
/* st3d_shade_fwd with lighting (R (B,3,3), trans (B,3): the cameras of the views) */
int st3d_shade_lit_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                       const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int T,
                       int F, int VT, const float *verts, const float *normals, const int32_t *faces, const float *R,
                       const float *trans, const float *light, int n_lights, int kind, float *rgb, float *mask,
                       st3d_stream_t stream);
/* -> grad_texture (T,T,3) accumulated (may be NULL), grad_bary (B,S,S,3) and grad_np (B,S,S,6) = per pixel d/dN, d/dP
 * (both or neither).  workspace NULL: float atomics; else (>= st3d_shade_bwd_det_workspace_bytes(T), 16-byte aligned,
 * grad_texture given) the fixed-point scatter of st3d_shade_bwd_det, its bound scaled by weight_bound >= max_c (A + D)_c
 * (e.g. max over entries and channels of |ka La| + |kd Ld|).
 * grad_np is written at covered pixels only (pix_to_face >= 0): elsewhere it keeps what the buffer held.  Its one
 * consumer, st3d_phong_scatter, reads covered fragments only.  The same holds per fragment for st3d_shade_soft_lit_bwd and
 * st3d_shade_ss_lit_bwd. */
int st3d_shade_lit_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                       const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                       int B, int S, int T, int F, int VT, const float *verts, const float *normals,
                       const int32_t *faces, const float *R, const float *trans, const float *light, int n_lights,
                       int kind, float weight_bound, float *grad_texture, float *grad_bary, float *grad_np,
                       void *workspace, size_t workspace_bytes, st3d_stream_t stream);
/* the same for the general soft kernels (per layer: grad_np (B,S,S,K,6)); det workspace
 * >= st3d_shade_soft_bwd_det_workspace_bytes(T) */
int st3d_shade_soft_lit_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                            const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S,
                            int T, int K, float sigma, float gamma, const float *background, const float *verts,
                            const float *normals, const int32_t *faces, const float *R, const float *trans,
                            const float *light, int n_lights, int kind, float *rgb, float *alpha,
                            st3d_stream_t stream);
int st3d_shade_soft_lit_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                            const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                            int B, int S, int T, int K, float sigma, float gamma, const float *background,
                            const float *verts, const float *normals, const int32_t *faces, const float *R,
                            const float *trans, const float *light, int n_lights, int kind, float weight_bound,
                            float *grad_texture, float *grad_bary, float *grad_zbuf, float *grad_dists,
                            float *grad_np, void *workspace, size_t workspace_bytes, st3d_stream_t stream);
/* grad_np of the lit backward (K layers per pixel, K = 1 for the specialised path) -> out (2,V,3) = [d/d(vertex
 * positions), d/d(vertex normals)] through N = sum b_i n_i, P = sum b_i v_i, summed over the views (world space); out is
 * overwritten.  workspace NULL: float atomics; else (>= st3d_phong_scatter_workspace_bytes) bitwise reproducible. */
size_t st3d_phong_scatter_workspace_bytes(int B, int V, int S);
int st3d_phong_scatter(const float *grad_np, const int32_t *pix_to_face, const float *bary, const int32_t *faces,
                       int B, int V, int F, int S, int K, float *out, void *workspace, size_t workspace_bytes,
                       st3d_stream_t stream);

/* ---- supersampled rendering: the fragments are rasterised at side a * S (a = 1..4, a * S <= 4096) and the loss sees the
 * a x a box-filtered image at side S.  For output pixel (y, x): s = c[ay][ax], then s = s + c[ay+j][ax+i] for the other
 * sub-pixels in row-major order, out = s / (float)(a * a) -- fp32, uncontracted, correctly rounded division; c is the colour
 * st3d_shade_fwd computes at the sub-pixel (white where there is no face).  coverage (B,1,S,S) is the same expression over
 * the 0/1 mask: a count over a^2, > 0 exactly where some sub-pixel is covered.  Backward: every sub-pixel of a block runs
 * st3d_shade_bwd's expressions with grad_rgb(y, x) / (float)(a * a) as its gradient.  S is the side of rgb / grad_rgb;
 * pix_to_face, bary, zbuf, dists and the per-pixel outputs grad_uv, grad_bary, grad_np are at side a * S.  Neither the
 * a * S image nor an a * S gradient is ever written.  a = 1 is the plain entry point. */
int st3d_shade_ss_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                      const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int a,
                      int T, int F, int VT, float *rgb, float *coverage, st3d_stream_t stream);
int st3d_shade_ss_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                      const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                      int B, int S, int a, int T, int F, int VT, float *grad_texture, float *grad_uv,
                      float *grad_bary, st3d_stream_t stream);
/* fixed point (workspace >= st3d_shade_bwd_det_workspace_bytes(T)): the bound pass runs over grad_rgb itself; for a > 1 the
 * values of a pixel none of whose sub-pixels holds a face (it deposits nothing) enter it with weight 0, so the result does
 * not depend on finite values there and a NaN or an infinity anywhere still comes out as NaN */
int st3d_shade_ss_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                          const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                          int B, int S, int a, int T, int F, int VT, float *grad_texture /* accumulated into */,
                          float *grad_uv, float *grad_bary, void *workspace, size_t workspace_bytes,
                          st3d_stream_t stream);
int st3d_shade_ss_lit_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                          const float *verts_uvs, const int32_t *faces_uvs, const float *texture, int B, int S, int a,
                          int T, int F, int VT, const float *verts, const float *normals, const int32_t *faces,
                          const float *R, const float *trans, const float *light, int n_lights, int kind, float *rgb,
                          float *coverage, st3d_stream_t stream);
int st3d_shade_ss_lit_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                          const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *texture,
                          int B, int S, int a, int T, int F, int VT, const float *verts, const float *normals,
                          const int32_t *faces, const float *R, const float *trans, const float *light, int n_lights,
                          int kind, float weight_bound, float *grad_texture, float *grad_bary, float *grad_np,
                          void *workspace, size_t workspace_bytes, st3d_stream_t stream);
/* the box filter alone, in (B,C,a*S,a*S) -> out (B,C,S,S) with the sum order and division above, and its transpose
 * grad_out (B,C,S,S) -> grad_in (B,C,a*S,a*S) = grad_out / (float)(a * a) at every sub-pixel (overwritten) */
int st3d_box_down_fwd(const float *in, int B, int C, int S, int a, float *out, st3d_stream_t stream);
int st3d_box_down_bwd(const float *grad_out, int B, int C, int S, int a, float *grad_in, st3d_stream_t stream);

/* apply_background, utils.py:19-30: out = img*mask + bg*(1-mask); bg (B,3,S,S) or, with
 * bg_batch == 1, one (3,S,S) image broadcast over the batch.  Optional grad path is the
 * same kernel applied to the gradient with bg = NULL (out = g*mask). */
int st3d_apply_background(const float *img, const float *mask, const float *bg, int bg_batch,
                          int B, int S, float *out, st3d_stream_t stream);

/* ------------------------------------------------------------------ VGG-19 features:
 * utils.py:48-52 (get_vgg) + style_transfer.py:10-27 (get_features).  conv3x3 pad 1 +
 * bias + ReLU on fp32 MFMA (v_mfma_f32_32x32x2_f32), maxpool 2x2. */

/* packed-weight sizes in floats for a (Cout,Cin,3,3) filter */
size_t st3d_conv3x3_packed_floats(int Cout, int Cin);
/* w (Cout,Cin,3,3) -> w_fwd [9][Cin4][CoutP] and w_dgrad [9][Cout4][CinP] (rotated 180 deg,
 * channel-transposed); either output may be NULL.  Both buffers hold st3d_conv3x3_packed_floats floats, the larger of the
 * two layouts (Cin4, Cout4: rounded up to 4; CoutP, CinP: to 128); the floats behind a pack's own layout are neither
 * written here nor read by any kernel. */
int st3d_conv3x3_pack(const float *w, int Cout, int Cin, float *w_fwd, float *w_dgrad,
                      st3d_stream_t stream);
/* y = relu?(conv3x3(x, w) + bias): x (N,Cin,H,W), y (N,Cout,H,W) */
int st3d_conv3x3_fwd(const float *x, const float *w_fwd_packed, const float *bias, float *y,
                     int N, int Cin, int Cout, int H, int W, int relu, st3d_stream_t stream);
/* The 3-channel forward (conv1_1: one workgroup per 8 x 128-pixel tile, tiles numbered image-major, then row-major;
 * st3d_conv1_skip_tiles of them) over the tiles whose byte in tile_skip is 0: y keeps what it held at the others, the
 * computed tiles are bitwise st3d_conv3x3_fwd's.  Any other shape is ST3D_E_INVALID.  st3d_conv1_skip_build: skip = 1 where
 * cover (N,H,W bytes, non-zero = covered) holds nothing in the tile +- 1, i.e. every 3x3 window of the tile sees background
 * (or the zero padding) only -- such a tile's output does not change while the background colour and the weights stay. */
size_t st3d_conv1_skip_tiles(int N, int H, int W);
int st3d_conv1_skip_build(const uint8_t *cover, int N, int H, int W, uint8_t *skip, st3d_stream_t stream);
int st3d_conv3x3_fwd_skip(const float *x, const float *w_fwd_packed, const float *bias, float *y, int N, int Cin, int Cout,
                          int H, int W, int relu, const uint8_t *tile_skip, st3d_stream_t stream);
/* gx = conv3x3^T(mask(gy)): gradient w.r.t. the conv INPUT (weights are frozen,
 * utils.py:50-51: no wgrad).  gy (N,Cout,H,W) is the gradient w.r.t. the POST-ReLU output;
 * act (same shape, the saved post-ReLU output) gates it (act>0) when non-NULL. */
int st3d_conv3x3_dgrad(const float *gy, const float *act, const float *w_dgrad_packed, float *gx,
                       int N, int Cin, int Cout, int H, int W, st3d_stream_t stream);
/* The bottom of the VGG backward fused (csrc/tap0.hip): gx (N,3,H,W) = conv1_1^T(gate(gy + coef * D act)) where act
 * (N,64,H,W) is the saved relu1_1 output (gate: act > 0), gy (N,64,H,W) the gradient arriving from conv1_2 (NULL = none)
 * and D (N,64,64) the style-loss difference Gram of the relu1_1 tap (NULL = no tap) -- what st3d_gram_bwd(accumulate)
 * followed by st3d_conv3x3_dgrad compute (autograd of losses.py:36-39 + second_approach.py:188), in one pass over gy and
 * act.  w_dgrad_packed: conv1_1's dgrad pack of st3d_conv3x3_pack.  workspace: st3d_conv1_bwd_workspace_bytes. */
int st3d_conv1_bwd_supported(int H, int W);
size_t st3d_conv1_bwd_workspace_bytes(int N, int H, int W);
int st3d_conv1_bwd(const float *gy, const float *act, const float *D, float coef, const float *w_dgrad_packed,
                   void *workspace, size_t workspace_bytes, float *gx, int N, int H, int W, st3d_stream_t stream);
/* st3d_conv1_bwd for a consumer that reads gx at the pixels of mask (N,H,W bytes, non-zero = read) only: gx is bitwise
 * st3d_conv1_bwd's at those pixels and exactly 0 elsewhere.  seg (N,H,W/64 bytes) marks the 64-pixel row segments that
 * touch dilate(mask, 1) (st3d_need_build): gy is read, and the tap planes are computed, in those segments only.
 * W % 64 == 0. */
int st3d_conv1_bwd_masked(const float *gy, const float *act, const float *D, float coef, const float *w_dgrad_packed,
                          void *workspace, size_t workspace_bytes, float *gx, int N, int H, int W, const uint8_t *seg,
                          const uint8_t *mask, st3d_stream_t stream);
/* The bottom pass of the guided style loss: t = gy + coef * D (w0[p] act[:,p]), w0 (N,H,W) one weight per pixel applied to
 * the activation before the first product; the ReLU gate is the sign of the unweighted activation.  With D NULL there is nothing to weight (st3d_conv1_bwd's result).
 * seg and mask both NULL: st3d_conv1_bwd's form; both given: st3d_conv1_bwd_masked's (W % 64 == 0). */
int st3d_conv1_bwd_weighted(const float *gy, const float *act, const float *D, float coef, const float *w_dgrad_packed,
                            void *workspace, size_t workspace_bytes, float *gx, int N, int H, int W, const float *w0,
                            const uint8_t *seg, const uint8_t *mask, st3d_stream_t stream);
/* As above, but gy is given at POOLED resolution (N,Cout,H/2,W/2) together with the pool's
 * argmax (uint8 0..3 = dy*2+dx) and pooled values: fuses max-unpool + ReLU gate into the load. */
int st3d_conv3x3_dgrad_unpool(const float *gy_pooled, const uint8_t *pool_idx, const float *pooled,
                              const float *w_dgrad_packed, float *gx, int N, int Cin, int Cout,
                              int H, int W, st3d_stream_t stream);
/* Winograd F(2x2,3x3) variants of the three conv entry points above (exact-fp32 MFMA products,
 * 2.25x fewer of them); for Cin % 8 == 0, Cout % 64 == 0, H even, W % 4 == 0 -- every VGG
 * layer but conv1_1.  u_fwd / u_dgrad = G g G^T in the kernel's MFMA-operand order (st3d_wino_pack).
 * st3d_wino_fwd can fuse the following MaxPool2d(2,2): y_pooled (N,Cout,H/2,W/2) + pool_idx
 * (either NULL = no pooling); y may then be NULL to skip the full-resolution store. */
int st3d_wino_supported(int Cin, int Cout, int H, int W);
size_t st3d_wino_packed_floats(int Cout, int Cin);
int st3d_wino_pack(const float *w, int Cout, int Cin, float *u_fwd, float *u_dgrad, st3d_stream_t stream);
int st3d_wino_fwd(const float *x, const float *u_fwd, const float *bias, float *y, float *y_pooled,
                  uint8_t *pool_idx, int N, int Cin, int Cout, int H, int W, int relu, st3d_stream_t stream);
int st3d_wino_dgrad(const float *gy, const float *act, const float *u_dgrad, float *gx, int N, int Cin,
                    int Cout, int H, int W, st3d_stream_t stream);
int st3d_wino_dgrad_unpool(const float *gy_pooled, const uint8_t *pool_idx, const float *pooled,
                           const float *u_dgrad, float *gx, int N, int Cin, int Cout, int H, int W,
                           st3d_stream_t stream);
/* One link of the backward chain with the ReLU gates moved to the PRODUCER of each gradient, so that the 8-64 stages of
 * the consumer's K loop stream one operand instead of two or three (measured 3-13 % per launch):
 *   input : gy, full resolution gated by act (NULL = gy is already gated), or -- pool_idx != NULL -- at pooled resolution,
 *           un-pooled through pool_idx and gated by pooled > 0 (pooled == NULL = already gated);
 *   output: gx = conv^T(...), zeroed where out_gate (N,Cin,H,W: the conv's own forward input, post-ReLU or pool output)
 *           is <= 0 when out_gate != NULL -- i.e. gx is handed on already gated for the next link.  With add_target
 *           (same shape, needs out_gate) the content-loss gradient add_coef * (out_gate - add_target) of that tensor
 *           (losses.py:24-28; what st3d_axpy_diff adds) joins gx before the gate, in the same store. */
int st3d_wino_dgrad_chain(const float *gy, const float *act, const uint8_t *pool_idx, const float *pooled,
                          const float *u_dgrad, const float *out_gate, const float *add_target, float add_coef,
                          float *gx, int N, int Cin, int Cout, int H, int W, st3d_stream_t stream);
/* The same convolutions as Winograd F(4x4,3x3) (csrc/wino43.hip, round 3): 2.25 instead of 4 MFMA-multiplies per output
 * pixel, fp32 throughout (on VGG's real operands and randn <= 1.9e-5 of max|ref| against an fp64 convolution, <= 122 u M per
 * element: tests/test_gpu_conv_accuracy.py).  Shapes: Cin % 64 == 0,
 * Cout % 64 == 0 (what st3d_wino43_pack accepts), and H % 4 == 0 with W % 64 == 0 or H % 8 == 0 with W % 32 == 0
 * (the workgroup's step is 4 x 64 or 8 x 32 pixels), each tensor < 2^31 bytes per image
 * (st3d_wino43_supported).  Own filter pack (36 floats per weight).  One persistent workgroup per CU.
 * st3d_wino43_dgrad_chain takes an already gated gradient (or, with pool_idx, the pooled-resolution gradient) exactly as
 * st3d_wino_dgrad_chain does with act == pooled == NULL. */
int st3d_wino43_supported(int Cin, int Cout, int H, int W);
size_t st3d_wino43_packed_floats(int Cout, int Cin);
int st3d_wino43_pack(const float *w, int Cout, int Cin, float *u_fwd, float *u_dgrad, st3d_stream_t stream);
int st3d_wino43_fwd(const float *x, const float *u_fwd, const float *bias, float *y, float *y_pooled, uint8_t *pool_idx,
                    int N, int Cin, int Cout, int H, int W, int relu, st3d_stream_t stream);
int st3d_wino43_dgrad_chain(const float *gy, const uint8_t *pool_idx, const float *u_dgrad, const float *out_gate,
                            const float *add_target, float add_coef, float *gx, int N, int Cin, int Cout, int H, int W,
                            st3d_stream_t stream);
/* The output tiles of a F(4x4,3x3) launch on an H x W map: rows x cols pixels (4 x 64 or 8 x 32), numbered
 * (n * (H / rows) + ty) * (W / cols) + tx.  Returns 0 (and zeros) where the kernel does not cover the map. */
int st3d_wino43_tile_geometry(int H, int W, int *rows, int *cols);
/* st3d_wino43_dgrad_chain over the first *n_active entries of tile_list only (both in DEVICE memory, tile numbers
 * ascending): a listed tile of gx is bitwise what the unlisted call writes, the other tiles are not written. */
int st3d_wino43_dgrad_chain_tiles(const float *gy, const uint8_t *pool_idx, const float *u_dgrad, const float *out_gate,
                                  const float *add_target, float add_coef, float *gx, int N, int Cin, int Cout, int H, int W,
                                  const int *tile_list, const int *n_active, st3d_stream_t stream);
/* Need propagation (csrc/need.hip): the only consumer of the perceptual loss's image gradient, the render backward, reads
 * it at the pixels of mask (N,S,S bytes, non-zero = read; 16-byte aligned) only.  Bottom-up, what the last launches of the
 * VGG backward then have to produce:
 *   level 1  seg (N,S,S/64 bytes): 1 for the 64-pixel row segments that touch dilate(mask, 1) (st3d_conv1_bwd_masked)
 *   level 2  list1 / counts[0]: the output tiles of the conv1_2 input gradient (geometry of an S x S map) that hold an
 *            active segment
 *   level 3  list2 / counts[1]: the output tiles of the conv2_1 input gradient (geometry of an S/2 x S/2 map) that hold a
 *            pooled pixel of the 2x2 OR of dilate(union of the level-2 tiles, 1)
 * Lists are ascending, images outermost, and sized for every tile; they and the counts stay in device memory.
 * st3d_need_levels(S): how many levels exist at this size (0 when S % 64 != 0).  Ordered prefix-sum compaction, no atomics. */
int st3d_need_levels(int S);
size_t st3d_need_workspace_bytes(int N, int S);      /* one flag byte per tile of levels 2 and 3 */
int st3d_need_build(const uint8_t *mask, int N, int S, int levels, uint8_t *seg, void *workspace, size_t workspace_bytes,
                    int *list1, int *list2, int *counts, st3d_stream_t stream);
/* Need propagation per 4x4 block (csrc/need.hip): an F(4x4,3x3) launch computes each aligned 4x4 output block from that
 * block's own 6x6 patch alone, so what list k's launch has to get right is B_k = block4(need_k), and what it reads is
 * need_k+1 = dilate(B_k, 1) clipped to the map (through the 2x2 OR where the launch un-pools its input); need_0 =
 * dilate(mask, 1).  Lists 0 .. 5: the input gradients of conv1_2 (S x S), conv2_1, conv2_2 (S/2), conv3_1, conv3_2, conv3_3
 * (S/4).  list k holds the tiles that hold a block of B_k, in the geometry tile_cols[k] (host array; 64 = 4 x 64 pixels, 32 =
 * 8 x 32, 0 or tile_cols == NULL = st3d_wino43_tile_geometry's), ascending, st3d_need_blocks_tiles(N, S, k) entries long;
 * counts[k] the number listed.  lists: HOST array of nlists device pointers.  seg as st3d_need_build.  Device memory
 * throughout, no atomics.  st3d_need_blocks_lists(S): how many lists exist at this size (0: not covered).
 * tile_cols[k] = 16: strips.  list k holds the strips of 4 x 16 pixels, (n * strips_y + sy) * strips_x + sx, that hold a block
 * of B_k, ascending within an image, FOUR entries to a workgroup step, every image padded with -1 to whole steps; counts[k] =
 * steps.  The list is st3d_need_blocks_entries(N, S, k, 16) = 4 st3d_need_blocks_tiles entries long and 16-byte aligned. */
#define ST3D_NEED_MAX_LISTS 6
int st3d_need_blocks_lists(int S);
size_t st3d_need_blocks_tiles(int N, int S, int k);
size_t st3d_need_blocks_entries(int N, int S, int k, int tile_cols);
size_t st3d_need_blocks_workspace_bytes(int N, int S);
/* gram_list / gram_count (device; NULL = not wanted): the 64-pixel runs of the (S/2)^2 map that meet need_2, the pixels at
 * which the conv2_1 input gradient reads the gradient of relu2_1 -- what st3d_gram_bwd_gated_segs takes; numbered image *
 * runs per image + run, st3d_need_blocks_gram_runs(N, S) entries (0: S/2 is no multiple of 64, no such list); nlists >= 2. */
size_t st3d_need_blocks_gram_runs(int N, int S);
int st3d_need_blocks_build(const uint8_t *mask, int N, int S, int nlists, const int *tile_cols, uint8_t *seg, void *workspace,
                           size_t workspace_bytes, int *const *lists, int *counts, int *gram_list, int *gram_count,
                           st3d_stream_t stream);
/* The gated Gram backward (st3d_gram_bwd_gated; with q: st3d_gram_bwd_weighted, gated) over the first *seg_count entries of
 * seg_list only (device memory; entry = image * (HW / 64) + 64-pixel run).  C = 128 (st3d_gram_bwd_segs_supported).  A listed
 * run of gfeat is bitwise what the full launch writes; the other runs are not touched. */
int st3d_gram_bwd_segs_supported(int C, int HW);
int st3d_gram_bwd_gated_segs(const float *D, const float *feat, const float *q, int B, int C, int HW, float coef, int accumulate,
                             const int *seg_list, const int *seg_count, float *gfeat, st3d_stream_t stream);
/* st3d_wino43_dgrad_chain_tiles / st3d_wino43_fwd_tiles with the tile geometry as an argument: tile_cols = 64 (4 x 64 pixels,
 * W % 64 == 0) or 32 (8 x 32 pixels, H % 8 == 0 and W % 32 == 0); tile_list numbers the tiles of THAT geometry.  0 = the
 * geometry of st3d_wino43_tile_geometry.  The input-gradient chain also takes tile_cols = 16: tile_list (16-byte aligned) holds
 * FOUR entries per step, each a strip of 4 x 16 pixels (n * H/4 + sy) * W/16 + sx or -1 (none), all of one image, anywhere in
 * it; *n_active counts steps.  Every block of a listed strip is bitwise the unlisted call's, nothing else is written. */
int st3d_wino43_dgrad_chain_tiles_geo(const float *gy, const uint8_t *pool_idx, const float *u_dgrad, const float *out_gate,
                                      const float *add_target, float add_coef, float *gx, int N, int Cin, int Cout, int H, int W,
                                      int tile_cols, const int *tile_list, const int *n_active, st3d_stream_t stream);
int st3d_wino43_fwd_tiles_geo(const float *x, const float *u_fwd, const float *bias, float *y, float *y_pooled, uint8_t *pool_idx,
                              int N, int Cin, int Cout, int H, int W, int relu, int tile_cols, const int *tile_list,
                              const int *n_active, st3d_stream_t stream);
/* The plain forward over a strip list: strip_list as tile_list with tile_cols = 16 above, *n_steps counts steps.  bias (may be
 * NULL) and relu as st3d_wino43_fwd; every block of a listed strip of y is bitwise st3d_wino43_fwd's, nothing else is written.
 * There is no fused pool over strips (st3d_wino43_fwd_tiles_geo refuses tile_cols = 16 with y_pooled, and with bias or relu). */
int st3d_wino43_fwd_strips(const float *x, const float *u_fwd, const float *bias, float *y, int N, int Cin, int Cout, int H,
                           int W, int relu, const int *strip_list, const int *n_steps, st3d_stream_t stream);
/* Kept lists (csrc/need.hip): which output blocks of the forward launches conv1_2 .. conv3_3 (lists 0 .. 5, the maps of
 * st3d_need_blocks_build) can differ between two calls whose images differ only where cover (N,S,S bytes, 16-byte aligned) is
 * non-zero.  conv1_1 is per pixel and an F(4x4,3x3) launch per aligned 4x4 block, so K_0 = block4(dilate(cover, 2)) and
 * K_k+1 = block4(dilate(K_k, 1)), through the 2x2 OR behind a fused pool.  Lists first .. nlists - 1 are made, each holding the
 * tiles (tile_cols[k] = 64 / 32 / 0) or strips (16) with a block of K_k, in the formats, sizes and alignment of
 * st3d_need_blocks_build; lists: HOST array of nlists device pointers (entries below first are not read), counts[k] the count
 * of list k.  workspace: st3d_need_blocks_workspace_bytes(N, S).  Two launches, no atomics. */
int st3d_kept_build(const uint8_t *cover, int N, int S, int first, int nlists, const int *tile_cols, void *workspace,
                    size_t workspace_bytes, int *const *lists, int *counts, st3d_stream_t stream);
/* st3d_wino43_fwd over the first *n_active entries of tile_list only (as above): y, y_pooled and pool_idx of a listed tile
 * are bitwise what st3d_wino43_fwd writes, nothing else is written. */
int st3d_wino43_fwd_tiles(const float *x, const float *u_fwd, const float *bias, float *y, float *y_pooled, uint8_t *pool_idx,
                          int N, int Cin, int Cout, int H, int W, int relu, const int *tile_list, const int *n_active,
                          st3d_stream_t stream);
/* Flat-field lists (csrc/flat.hip): a hard render holds its background colour bit for bit at most pixels, and a conv output
 * tile whose input patch sees only the field that colour produces equals every other such tile of its border class.
 * imgs (N,3,S,S; 16-byte aligned), color: 3 floats in DEVICE memory.  V0 = the pixel differs from color in any channel,
 * compared as bits (NaN varies); conv1_1 maps V to dilate(V, 1), a Winograd conv to the aligned 4x4 output blocks that
 * meet dilate(V, 1) (a block is rounded from its whole 6x6 patch), a 2x2 pool to the 2x2 OR; a tile is varying iff its input
 * patch (tile +- 1, clipped) meets the V of its input.  Launches: 1 conv1_2 (S x S map), 2 conv2_1, 3 conv2_2 (S/2 x S/2),
 * tiles numbered as st3d_wino43_tile_geometry.  list_k / counts[k-1]: the varying tiles plus, per class (min(ty,2),
 * min(TY-1-ty,2), min(tx,2), min(TX-1-tx,2)) of non-varying tiles, its lowest-indexed member over the whole batch; ascending.
 * map_k: per tile its class representative, -1 for listed tiles.  Lists and maps are sized st3d_flat_tiles(N, S, k - 1);
 * everything stays in device memory.  levels = how many launches (1..st3d_flat_levels(S): 3, or 0 when S % 64 != 0).
 * Ordered compaction, no atomics to global memory.
 * st3d_flat_fill: every unlisted tile of y (N,C,H,W) / y_pooled / pool_idx (N,C,H/2,W/2; any may be NULL) takes its
 * representative's block; listed tiles are not touched.  Runs behind the listed conv launch on the same stream. */
int st3d_flat_levels(int S);
int st3d_flat_tiles(int N, int S, int launch /*0..2*/);
size_t st3d_flat_workspace_bytes(int N, int S);
int st3d_flat_build(const float *imgs, const float *color, int N, int S, int levels, void *workspace, size_t workspace_bytes,
                    int *list1, int *map1, int *list2, int *map2, int *list3, int *map3, int *counts, st3d_stream_t stream);
int st3d_flat_fill(const int *tile_map, float *y, float *y_pooled, uint8_t *pool_idx, int N, int C, int H, int W,
                   st3d_stream_t stream);
/* st3d_flat_build with V0 taken from a coverage mask (N,S,S bytes, non-zero = covered = varying; 16-byte aligned) instead of
 * the pixels: the lists depend on the geometry alone, so views that do not move build them once.  They list a superset of
 * the pixel lists' tiles provided every uncovered pixel holds the background colour bit for bit -- the caller's premise.
 * st3d_flat_check_cover tests it: *bad (device int) = 1 if a pixel of imgs outside cover differs from color, else 0 (it
 * uses the V0 plane of the workspace, which st3d_flat_build_cover leaves alone). */
int st3d_flat_build_cover(const uint8_t *cover, int N, int S, int levels, void *workspace, size_t workspace_bytes, int *list1,
                          int *map1, int *list2, int *map2, int *list3, int *map3, int *counts, st3d_stream_t stream);
int st3d_flat_check_cover(const float *imgs, const float *color, const uint8_t *cover, int N, int S, void *workspace,
                          size_t workspace_bytes, int *bad, st3d_stream_t stream);
/* MaxPool2d(2,2): y (N,C,H,W) -> p (N,C,H/2,W/2) (+ argmax idx, may be NULL) */
int st3d_maxpool2x2_fwd(const float *y, float *p, uint8_t *idx, int N, int C, int H, int W,
                        st3d_stream_t stream);

/* ------------------------------------------------------------------ Gram / losses:
 * style_transfer.py:31-35 (gram_matrix), losses.py:31-42 */

size_t st3d_gram_workspace_bytes(int B, int C, int HW);
/* gram (B,C,C) = F F^T, F = feat (B,C,HW); unnormalised; split-K fp32 MFMA + ordered
 * (deterministic) slab reduction. */
int st3d_gram_fwd(const float *feat, int B, int C, int HW, void *workspace, size_t workspace_bytes,
                  float *gram, st3d_stream_t stream);
/* The Grams of ALL style layers of a step (losses.py:34-37 loops over them; style_transfer.py:47-49,
 * 66-69 likewise) in one launch pair: items is a HOST array (<= 8), every item is one
 * st3d_gram_fwd problem; workspace >= st3d_gram_multi_workspace_bytes(items, count), 256-byte
 * aligned (each layer has its own slab region: they run concurrently).  Bitwise the results of
 * st3d_gram_fwd per item.  ST3D_GRAM_MULTI=0 runs the items one by one (A/B). */
typedef struct st3d_gram_item {
    const float *feat;   /* (B, C, HW) */
    float *gram;         /* (B, C, C) */
    int B, C, HW;
} st3d_gram_item;
size_t st3d_gram_multi_workspace_bytes(const st3d_gram_item *items, int count);
int st3d_gram_fwd_multi(const st3d_gram_item *items, int count, void *workspace, size_t workspace_bytes,
                        st3d_stream_t stream);
/* gfeat (B,C,HW) (+)= coef * (D F) with D (B,C,C) symmetric (D = G - S); accumulate != 0 adds
 * into gfeat. */
int st3d_gram_bwd(const float *D, const float *feat, int B, int C, int HW, float coef,
                  int accumulate, float *gfeat, st3d_stream_t stream);
/* the same, then gfeat = 0 where feat <= 0 (feat is post-ReLU: its ReLU gate, taken from the operand tile already in
 * LDS), so the gradient leaves already gated (see st3d_wino_dgrad_chain).  C % 32 == 0. */
int st3d_gram_bwd_gated(const float *D, const float *feat, int B, int C, int HW, float coef,
                        int accumulate, float *gfeat, st3d_stream_t stream);
/* ---- guided style loss (default off): the Gram of a tap taken over a guided region (Gatys et al. 2017, spatial control).
 * Guidance planes of a mask (n,1,S,S), fp32 in [0,1] (a render's 0/1 coverage), one per style tap l = 0..4:
 *   H_0 = S, H_{l+1} = H_l / 2 (floor);  a_0 = mask;
 *   a_{l+1}[y][x] = 0.25f * ((a_l[2y][2x] + a_l[2y][2x+1]) + (a_l[2y+1][2x] + a_l[2y+1][2x+1]));
 *   Sigma_l = sum_p a_l[p] per image (ordered two-stage reduction: bitwise reproducible; exact for 0/1 masks up to S = 4096);
 *   r_l = (float)(H_l^2) / Sigma_l, or 0 when Sigma_l is not > 0;   w_l = a_l r_l;   q_l = sqrtf(w_l)
 * (correctly rounded division and square root).  A value outside [0,1] is the caller's business: a negative one gives NaN.
 * st3d_guidance_build writes the q_l planes one after the other into q_out (st3d_guidance_floats(n, S) floats: level l is
 * (n, H_l, H_l) and starts n * (H_0^2 + .. + H_{l-1}^2) floats in) and Sigma into sums_out (5 x n floats, [l * n + image]);
 * partials: st3d_guidance_partials(n, S) floats of scratch.  S >= 16.  Two launches, no atomics, nothing allocated. */
size_t st3d_guidance_floats(int n, int S);
size_t st3d_guidance_partials(int n, int S);
int st3d_guidance_build(const float *mask, int n, int S, float *q_out, float *sums_out, float *partials,
                        st3d_stream_t stream);
/* ---- style regions (default off): the guidance planes of R regions of a mesh from the fragments of a render.  For region
 * r the level-0 plane is a_0 = 1 where pix_to_face (n,S,S; < 0 = no face) names a face f with face_region[f] == r, else 0
 * (background pixels and labels >= R belong to no region); everything after that is st3d_guidance_build's arithmetic in
 * its pairing and order.  q_out holds R blocks of st3d_guidance_floats(n, S) floats, block r laid out as
 * st3d_guidance_build lays out its q_out and bit for bit what it gives for that one-hot mask; sums_out is (R,5,n),
 * [(r * 5 + l) * n + image]; partials: st3d_region_planes_partials(n, S, R) floats of scratch.  One workgroup per 16 x 16
 * tile and image reads pix_to_face once and takes all regions through the five levels in LDS: no (n,R,S,S) mask exists
 * anywhere.  1 <= R <= 8, S >= 16, F >= 1; pix_to_face < F is the caller's guarantee (a larger index is read as no face).
 * Two launches, no atomics, nothing allocated. */
size_t st3d_region_planes_floats(int n, int S, int R);     /* R * st3d_guidance_floats(n, S); 0 for R outside 1..8 */
size_t st3d_region_planes_partials(int n, int S, int R);   /* R * st3d_guidance_partials(n, S) */
int st3d_region_planes(const int32_t *pix_to_face, const uint8_t *face_region, int n, int S, int F, int R, float *q_out,
                       float *sums_out, float *partials, st3d_stream_t stream);
/* The guided Gram  gram[b] = sum_p w[b][p] F[:,p] F[:,p]^T  computed as the Gram of q o F, q (B,HW) one plane of
 * st3d_guidance_build: both operand tiles are multiplied by q[p] on their way into LDS (no scaled copy of the activation
 * exists anywhere).  Workspace, splits, kernels' bodies and reduce are those of st3d_gram_fwd: symmetric bit for bit, and
 * q == 1 gives st3d_gram_fwd's bits.  NaN / Inf propagate as the products say (NaN under q = 0 stays NaN). */
int st3d_gram_fwd_weighted(const float *feat, const float *q, int B, int C, int HW, void *workspace,
                           size_t workspace_bytes, float *gram, st3d_stream_t stream);
/* All guided Grams of a step in one launch pair: q[i] (a HOST array of device pointers, parallel to items) is the plane
 * of items[i].  Workspace as st3d_gram_fwd_multi.  Bitwise the results of st3d_gram_fwd_weighted per item. */
int st3d_gram_fwd_multi_weighted(const st3d_gram_item *items, const float *const *q, int count, void *workspace,
                                 size_t workspace_bytes, st3d_stream_t stream);
/* Gradient of the guided style term: gfeat (B,C,HW) (+)= coef * q o (D (q o feat)), D (B,C,C) = G^ - S symmetric.  feat is
 * staged as it is and multiplied by q[n] twice, fl(q fl(q feat)), as the operand leaves LDS (a column of the product is a
 * column of that operand): the accumulators start from gfeat as in st3d_gram_bwd, and q == 1 gives its bits in every mode.
 * gated != 0 (C % 32 == 0): gfeat = 0 where feat <= 0 -- the gate is the sign of feat itself, so with accumulate the
 * gradient that arrived from the layers above passes wherever the ReLU was open, also under q = 0. */
int st3d_gram_bwd_weighted(const float *D, const float *feat, const float *q, int B, int C, int HW, float coef,
                           int accumulate, int gated, float *gfeat, st3d_stream_t stream);
/* loss_out[0] += scale * sum((a-b)^2) over n elements (b broadcast with period nb, nb | n);
 * if D != NULL also D = a - b.  Deterministic two-stage reduction through `partials`
 * (>= st3d_reduce_partials() floats). */
int st3d_reduce_partials(void);
int st3d_sqdiff_sum(const float *a, const float *b, size_t n, size_t nb, float scale, float *D,
                    float *partials, float *loss_out, st3d_stream_t stream);
/* Up to 8 squared-difference sums in one launch pair (the plan's loss tail): item k adds scale * sum((a - b)^2) over n
 * elements (b with period nb; D = a - b when non-NULL) into loss_out3[slot], slot in {0, 1, 2}; zero_first clears the
 * three slots first; combine != 0 then sets loss_out3[0] = content_weight * loss_out3[1] + style_weight * loss_out3[2]
 * (losses.py:41-44).  Every item keeps the decomposition and the summation tree of st3d_sqdiff_sum: same bits.
 * partials: count * st3d_reduce_partials() floats. */
typedef struct st3d_sqdiff_item {
    const float *a; const float *b; float *D;
    size_t n, nb;
    float scale;
    int slot;
} st3d_sqdiff_item;
int st3d_sqdiff_sum_multi(const st3d_sqdiff_item *items, int count, float *partials, float *loss_out3,
                          int zero_first, int combine, float style_weight, float content_weight,
                          st3d_stream_t stream);
/* content loss backward: g (+)= coef * (a - b)  */
int st3d_axpy_diff(const float *a, const float *b, size_t n, float coef, int accumulate, float *g,
                   st3d_stream_t stream);
/* the same, then g = 0 where a <= 0: a is the post-ReLU activation the gradient g belongs to, so g leaves already gated
 * (see st3d_wino_dgrad_chain) */
int st3d_axpy_diff_gated(const float *a, const float *b, size_t n, float coef, int accumulate, float *g,
                         st3d_stream_t stream);
/* masked MSE of losses.py:68-75 ('texture' branch): loss_out[0] = mean((r*m - t*m)^2) over
 * B*3*S*S; grad_r = 2*m*m*(r - t)/(B*3*S*S) (may be NULL). */
int st3d_masked_mse(const float *rendered, const float *target, const float *mask, int B, int S,
                    float *grad_rendered, float *partials, float *loss_out, st3d_stream_t stream);
/* masked anisotropic L1 total variation of losses.py:55-65 (compute_tv_loss; every call site in the reference is
 * commented out): images (B,C,H,W), masks (B,1,H,W); loss_and_mask_sum[0] = (sum |dI/dy| m m' + sum |dI/dx| m m') /
 * sum(masks), [1] = sum(masks); grad_images (same shape, may be NULL) = d loss / d images.  partials must hold
 * 2 * st3d_reduce_partials() floats. */
int st3d_tv_loss(const float *images, const float *masks, int B, int C, int H, int W, float *partials,
                 float *loss_and_mask_sum, float *grad_images, st3d_stream_t stream);
/* losses.py:48-51 (rgb_range_loss): loss_out[0] = sum relu(v - 1) + relu(-v); grad (may be NULL) = +1 / -1 / 0 */
int st3d_range_loss(const float *values, size_t n, float *partials, float *loss_out, float *grad, st3d_stream_t stream);

/* ------------------------------------------------------------------ mesh regularisers:
 * losses.py:84-87,93-96,112-115,121-124 -- F.mse_loss(verts, target), pytorch3d.loss
 * mesh_edge_loss (target length 0), mesh_laplacian_smoothing('uniform'), mesh_normal_consistency
 * for one mesh, forward + gradient in one call.  Topology is static and precomputed by the host:
 * edges (E,2) unique undirected; CSR vertex adjacency nbr_off (V+1), nbr_idx; pairs (P,4) =
 * (v0, v1, a, b) for every two faces sharing edge (v0,v1) with opposite vertices a, b; and the
 * inverse of `pairs`: pair_off (V+1), pair_ref = for each vertex the entries (pair * 4 + column)
 * of `pairs` that name it, ascending.  Every gradient is a per-vertex gather over these static
 * lists in a fixed order -- no float atomics, bitwise reproducible (round 3).
 * weights: host float[4] = {verts_mse, edge, laplacian, normal}.  scratch >=
 * st3d_mesh_reg_scratch_floats(V, P) floats, partials >= 4*st3d_reduce_partials() floats.
 * loss_out: device float[5] = {weighted sum, mse, edge, laplacian, normal} (unweighted terms).
 * grad_verts (V,3) += weighted gradient. */
size_t st3d_mesh_reg_scratch_floats(int V, int P);
int st3d_mesh_reg(const float *verts, const float *target_verts, int V, const int32_t *edges, int E,
                  const int32_t *nbr_off, const int32_t *nbr_idx, const int32_t *pairs, int P,
                  const int32_t *pair_off, const int32_t *pair_ref,
                  const float *weights, float *scratch, float *partials, float *loss_out,
                  float *grad_verts, st3d_stream_t stream);

/* The same four terms, loss_out layout and `grad_verts +=` with PyTorch3D's other two Laplacians and an edge target length
 * (DESIGN 7).  laplacian_method: 0 uniform, 1 cot, 2 cotcurv.  With, per face (v0,v1,v2), A=|v1-v2|, B=|v0-v2|, C=|v0-v1|,
 * s=(A+B+C)/2, area = sqrt(max(s(s-A)(s-B)(s-C), 1e-12)), cot_0 = (B^2+C^2-A^2)/(4 area) (cot_1, cot_2 alike), L symmetric with
 * L[v1,v2] += cot_0, L[v2,v0] += cot_1, L[v0,v1] += cot_2 over all faces, Lsum_i = sum_j L_ij, Asum_i = the areas of i's faces:
 *   cot:     r_i = (sum_j L_ij v_j) nw_i - v_i, nw_i = 1/Lsum_i where Lsum_i > 0, else Lsum_i itself
 *   cotcurv: r_i = (sum_j L_ij v_j - Lsum_i v_i) * 0.25 / Asum_i (0 where Asum_i is not > 0)
 * laplacian = (1/V) sum_i |r_i|; L, nw, Asum and Lsum are constants of the gradient, as in PyTorch3D.
 * edge_target_length t >= 0, finite: edge = (1/E) sum_e (|a-b| - t)^2, gradient direction 0 at |a-b| = 0.
 * At method 0 and t = 0 the launches and the bits are st3d_mesh_reg's.
 * Static lists beyond st3d_mesh_reg's (needed for method 1 / 2 only, else may be NULL), all host-built, every index in
 * range (nothing is checked on the device): faces (F,3); nbr_edge (2E) = for every slot of nbr_idx the row of `edges` it
 * stands for; CSR edge -> incident corners edge_off (E+1), edge_ref = face * 3 + (corner opposite the edge), ascending;
 * CSR vertex -> incident corners inc_off (V+1), inc_ref = face * 3 + corner, ascending.  Every sum is a gather over these
 * lists in list order: no float atomics, two runs are bit-equal.  The cot / target-length kernels compute in fp64 and round
 * each output once.  scratch >= st3d_mesh_reg_ex_scratch_floats(V, E, F, P) floats (0 for sizes the call refuses), 8-byte
 * aligned; partials as for st3d_mesh_reg.  ST3D_E_INVALID: null pointers, non-positive sizes, an unknown method, a negative
 * or non-finite t. */
size_t st3d_mesh_reg_ex_scratch_floats(int V, int E, int F, int P);
int st3d_mesh_reg_ex(const float *verts, const float *target_verts, int V, const int32_t *edges, int E,
                     const int32_t *nbr_off, const int32_t *nbr_idx, const int32_t *pairs, int P,
                     const int32_t *pair_off, const int32_t *pair_ref, const int32_t *faces, int F,
                     const int32_t *nbr_edge, const int32_t *edge_off, const int32_t *edge_ref,
                     const int32_t *inc_off, const int32_t *inc_ref, int laplacian_method, float edge_target_length,
                     const float *weights, float *scratch, float *partials, float *loss_out,
                     float *grad_verts, st3d_stream_t stream);

/* ------------------------------------------------------------------ Chamfer loss (csrc/chamfer.hip):
 * PyTorch3D's sample_points_from_meshes + knn_points(K=1) + chamfer_distance for ONE mesh and ONE pair of clouds.
 * Clouds are (P,3) fp32 with 1 <= P <= 2^20; every sum is ordered, in fp64, rounded once (no float atomics: two runs are
 * bit-equal).  ST3D_E_INVALID before any launch: null pointers, sizes out of range, a short or misaligned (8 bytes)
 * workspace / scratch.  Nothing is allocated.
 *
 * Nearest neighbour: for query x_i scan j = 0 .. P2-1, d = (dx dx + dy dy) + dz dz in fp32 (no contraction), j replaces the
 * best when d < best (best = +Inf, idx = 0 at the start: the lowest index wins among equals, a NaN target is never chosen).
 * dist[i] is recomputed from x_i and y[idx[i]] (a NaN query gives NaN).  The y range is split into `segments` runs of
 * ceil(ceil(P2 / tile) / segments) * tile points, each scanned by its own workgroups in LDS tiles of `tile` points; a second
 * pass takes the minimum over the runs in ascending order with the same d < best.  st3d_knn1_geometry reports tile and
 * segments of the launch st3d_knn1 makes for (P1, P2); workspace >= st3d_knn1_workspace_bytes (0 for refused sizes). */
int st3d_knn1_geometry(int P1, int P2, int *tile, int *segments);
size_t st3d_knn1_workspace_bytes(int P1, int P2);
int st3d_knn1(const float *x, const float *y, int P1, int P2, void *workspace, size_t workspace_bytes, int32_t *idx, float *dist,
              st3d_stream_t stream);
/* cdf (F) fp64: the inclusive scan, in a fixed tree, of area_f = |(v1 - v0) x (v2 - v0)| / 2 evaluated in fp64 from the fp32
 * vertices.  faces (F,3) int32, every index in range (checked by the caller).  scratch >= st3d_face_area_cdf_scratch_bytes. */
size_t st3d_face_area_cdf_scratch_bytes(int F);
int st3d_face_area_cdf(const float *verts, const int32_t *faces, int F, void *scratch, size_t scratch_bytes, double *cdf,
                       st3d_stream_t stream);
/* r (3,N) fp32 uniforms in [0,1), row 0 ascending.  face_idx[n] = the smallest f with cdf_f > (double)r0[n] * cdf_{F-1},
 * clamped to [0, F-1] (ascending in n); s = sqrtf(r1), w0 = 1 - s, w1 = s (1 - r2), w2 = s r2;
 * points[n] = (w0 a + w1 b) + w2 c per coordinate in fp32.  A total area cdf_{F-1} that is NaN or Inf (a NaN / Inf vertex)
 * draws no face: every point is NaN (face_idx = F-1), and with it the loss -- nothing aborts. */
int st3d_sample_points_fwd(const float *verts, const int32_t *faces, int F, const double *cdf, const float *r, int N,
                           float *points, int32_t *face_idx, st3d_stream_t stream);
/* grad_verts (V,3) += the gradient of <grad_points, points>: d a += w0 g, d b += w1 g, d c += w2 g (face choice and weights
 * are constants).  One (3,3) fp64 block per face in scratch (its samples found by binary search in the ascending face_idx,
 * added in order), then a gather per vertex over inc_off (V+1) / inc_ref (3F) = face * 3 + corner, in list order. */
size_t st3d_sample_points_bwd_scratch_bytes(int F);
int st3d_sample_points_bwd(const float *grad_points, const float *r, const int32_t *face_idx, int N, int F, int V,
                           const int32_t *inc_off, const int32_t *inc_ref, void *scratch, size_t scratch_bytes, float *grad_verts,
                           st3d_stream_t stream);
/* loss[0] = (float)((double)loss[0] + scale * sum_i dist[i]): the sum in fp64 in a fixed order, one rounding per call */
int st3d_chamfer_sum(const float *dist, int P, double scale, float *loss, st3d_stream_t stream);
/* One side of the Chamfer gradient, the indices being constants:
 *   grad_x[i] += c_self (x_i - y[nn[i]]) + c_other sum_{k: sorted[k] == i} (x_i - y[order[k]])
 * in fp64, rounded once.  nn (P1) = the neighbour of x_i in y; order (P2) / sorted (P2) = the indices and values of a stable
 * ascending sort of the neighbours of y_j in x (so the inner sum runs in ascending j).  nn may be NULL (no first term), or
 * order and sorted together (no second term).  Indices outside [0, P2) are skipped. */
int st3d_chamfer_bwd(const float *x, const float *y, int P1, int P2, const int32_t *nn, const int32_t *order,
                     const int32_t *sorted, double c_self, double c_other, float *grad_x, st3d_stream_t stream);

/* ------------------------------------------------------------------ NNFM style loss (csrc/nnfm.hip):
 * nearest-neighbour feature matching (Zhang et al., "ARF: Artistic Radiance Fields", ECCV 2022).  A render tap F (B,C,H,W),
 * fp32, post-ReLU, N = H W positions; a style tap S (Bs,C,Hs,Ws), M = Hs Ws, Bs = 1 (one style for every image) or B;
 * optional position weights w (B,N), each >= 0.  f_i / s_j: the C-vector at position i of image b / j of its style.
 *   norms     n_i = sqrtf(sum_c f_ic^2), the squares rounded and added in ascending c in fp32; f^_i = f_i / n_i; likewise s^_j.
 *   zeros     a zero vector has the unit copy 0: a zero style vector has similarity 0 with everything; a zero query
 *             (n_i = 0) has distance 1, index -1, gradient 0.  (ARF adds 1e-8 to the norm instead: a gradient of 1e8 at 0.)
 *   search    sim_ij = f^_i . s^_j, ONE fp32 fma chain in ascending c starting from 0 (the fp32 MFMA computes exactly that).
 *             j ascending from best = -Inf, idx = 0; j replaces the best when sim_ij > best: the lowest index wins among
 *             equals, a NaN style vector is never chosen, a NaN query keeps index 0 and gets a NaN distance.
 *   distance  d_i = 1 - sim_{i,idx_i}.  Positions with w_i = 0 are inactive: d_i = 0, idx_i = -1, gradient exactly 0, no search.
 *   loss      L_b = sum_i w_i d_i / sum_i w_i (w = 1 without weights), both sums in fp64 in a fixed order; an image with
 *             sum w = 0 contributes 0 and receives no gradient; L = inv_denom sum_b L_b, rounded once (inv_denom = 1 / the
 *             batch the mean divides by: B, or the global batch when views are sharded).
 *   gradient  indices and w are constants, S gets none:
 *             dL/df_i = -g (w_i inv_denom / (W_b n_i)) (s^_j - sim_ij f^_i), j = idx_i, W_b = sum_i w_i, in fp64, rounded once.
 * Sizes: 1 <= C <= 512, 1 <= N, M <= 2^20, 1 <= B <= 65535, Bs in {1, B}; anything else is ST3D_E_INVALID before any launch.
 * No float atomics anywhere: two runs are bit-equal.
 * geometry: the launch st3d_nnfm_search makes -- query tiles of tile_q positions, style tiles of tile_s positions, the style
 * range cut into `segments` runs of ceil(ceil(M / tile_s) / segments) tiles; the runs' maxima are merged in ascending order
 * with the same strict >.  workspace: segments * B * N * 8 bytes, 8-byte aligned, contents never read before written. */
int st3d_nnfm_geometry(int N, int M, int C, int *tile_q, int *tile_s, int *segments);
size_t st3d_nnfm_workspace_bytes(int B, int N, int M, int C);
/* x (B,C,M) -> xhat (B,C,M) (NULL: norms only), norm (B,M) */
int st3d_nnfm_normalise(const float *x, int B, int C, int M, float *xhat, float *norm, st3d_stream_t stream);
/* feat_hat (B,C,N) / feat_norm (B,N) and style_hat (Bs,C,M) from st3d_nnfm_normalise; weights (B,N) or NULL
 * -> idx (B,N), dist (B,N).  Query tiles without an active position are skipped. */
int st3d_nnfm_search(const float *feat_hat, const float *feat_norm, const float *style_hat, const float *weights, int B, int Bs,
                     int C, int N, int M, void *workspace, size_t workspace_bytes, int32_t *idx, float *dist,
                     st3d_stream_t stream);
/* loss[0] = L (overwritten), wsum[b] = W_b (B doubles): one workgroup, fp64, a fixed tree per image, the images in order.
 * (st3d_chamfer_sum has no weights and no per-image quotient.) */
int st3d_nnfm_sum(const float *dist, const float *weights, int B, int N, double inv_denom, float *loss, double *wsum,
                  st3d_stream_t stream);
/* grad_feat (B,C,N), every element written once (exact zeros at inactive positions, zero queries and images with W_b = 0);
 * feat is the tap itself (its norm is recomputed in fp64), sim is read back as 1 - dist; grad_out: the incoming scalar g on the device (NULL = 1). */
int st3d_nnfm_bwd(const float *feat, const float *style_hat, const int32_t *idx, const float *dist,
                  const float *weights, const double *wsum, const float *grad_out, int B, int Bs, int C, int N, int M,
                  double inv_denom, float *grad_feat, st3d_stream_t stream);

/* ------------------------------------------------------------------ sliced Wasserstein style loss (csrc/swd.hip):
 * Heitz, Vanhoey, Chambon, Belcour, "A Sliced Wasserstein Loss for Neural Texture Synthesis", CVPR 2021.  A render tap
 * F (B,C,H,W), fp32, post-ReLU, N = H W positions; a style tap S (Bs,C,Hs,Ws), M = Hs Ws, Bs = 1 or B; K directions V (K,C),
 * unit rows, constants of the gradient; optional position weights w (B,N), each >= 0.  Position i of image b is ACTIVE iff
 * w_bi > 0 (without weights every position is); the active positions are unweighted among themselves; n_b = their number.
 *   projection  p_kbi = sum_c V_kc F_bci, likewise t_kj for the style: ONE fp32 fma chain in ascending c starting from 0 (what
 *               the fp32 MFMA computes), never split over c, so a value does not depend on the tile it fell into and two
 *               positions with equal feature vectors get bit-equal projections.
 *   order       each row (b,k) is sorted ascending by the triple (inactive, key, index).  key = the order-preserving map of
 *               the fp32 bits to uint32 (all bits flipped if the sign bit is set, else the sign bit flipped: -0 before +0);
 *               every NaN is first replaced by 0x7FC00000 and so sorts after +Inf.  The triple is a total order: the result is
 *               unique whatever algorithm and tiling produce it.  sorted (B,K,N) fp32 holds the original values (NaNs as they
 *               came), perm (B,K,N) int32 the position that has each rank, count (B) int32 = n_b.  The style rows are sorted
 *               the same way, without weights or perm.
 *   matching    rank r < n_b meets the style quantile j(r) = ((2r+1) M) / (2 n_b) in integer arithmetic (the nearest-neighbour
 *               resampling of the sorted style row to n_b samples; j(r) = r when n_b = M).
 *   loss        L_b = (1 / (K n_b)) sum_k sum_{r<n_b} (sorted_kbr - tsorted_{k,j(r)})^2, differences, squares and sums in fp64
 *               in a fixed order; L = inv_denom sum_b L_b, rounded once.  An image with n_b = 0 adds 0 and gets no gradient.
 *   gradient    perm, V and w are constants, S gets none:
 *               dL/dp_{k,b,perm[r]} = g 2 inv_denom / (K n_b) (sorted_kbr - tsorted_{k,j(r)}) for r < n_b, in fp64, rounded
 *               once; an exact +0 at inactive positions and in images with n_b = 0; every element of gproj (B,K,N) is written
 *               exactly once, no atomics.  dL/dF_bci = sum_k V_kc gproj_kbi is st3d_swd_project again with V^T as the matrix.
 * NaN and Inf propagate as the expressions say.  Two runs are bit-equal.
 * Every entry point checks its arguments on the host: a bad size or a null pointer is ST3D_E_INVALID with nothing launched;
 * nothing allocates inside. */
/* out_brn = sum_q a_rq x_bqn, the chain above.  x (B,Q,N), a (R,Q), out (B,R,N); 1 <= Q, R <= 512, 1 <= N <= 2^20,
 * 1 <= B <= 65535; every offset is 64-bit. */
int st3d_swd_project(const float *x, const float *a, int B, int Q, int R, int N, float *out, st3d_stream_t stream);
/* the launch st3d_swd_sort makes for rows of N positions: a bitonic network on rows padded to a power of two P >= N; every
 * stride below `block` runs in LDS on `block` consecutive words, `passes` = the launches that take the strides >= block on
 * tiles strided in memory, one per level of the network above the block: log2(P / block), 0 when P <= block. */
int st3d_swd_geometry(int N, int *block, int *passes);
/* B K P 8 bytes when N > block, else 0 (the workspace may then be NULL); 0 for sizes st3d_swd_sort refuses */
size_t st3d_swd_workspace_bytes(int B, int K, int N);
/* proj (B,K,N), weights (B,N) or NULL -> sorted (B,K,N), perm (B,K,N) or NULL, count (B) or NULL.  1 <= K <= 512; workspace
 * 8-byte aligned, contents never read before written. */
int st3d_swd_sort(const float *proj, const float *weights, int B, int K, int N, void *workspace, size_t workspace_bytes,
                  float *sorted, int32_t *perm, int32_t *count, st3d_stream_t stream);
/* loss[0] = L (overwritten).  tsorted (Bs,K,M).  One fp64 sum per row (thread t of 256 adds r = t, t + 256, ... then a fixed
 * tree), then one workgroup adds the rows of each image the same way and the images in order: the tree is the same whatever
 * the launch.  workspace: B K doubles for the row sums, 8-byte aligned. */
int st3d_swd_loss(const float *sorted, const int32_t *count, const float *tsorted, int B, int Bs, int K, int N, int M,
                  double inv_denom, void *workspace, size_t workspace_bytes, float *loss, st3d_stream_t stream);
/* gproj (B,K,N): a scatter through perm with one writer per element; grad_out: the incoming scalar g on the device (NULL = 1) */
int st3d_swd_bwd(const float *sorted, const int32_t *perm, const int32_t *count, const float *tsorted, const float *grad_out,
                 int B, int Bs, int K, int N, int M, double inv_denom, float *gproj, st3d_stream_t stream);

/* ------------------------------------------------------------------ texture pyramid (csrc/texpyr.hip):
 * the texture map (T,T,3) as the sum of L maps of sides T_l = T / 2^l, each upsampled to T x T.  `params` is one flat
 * fp32 tensor of st3d_texpyr_numel(T, L) = 3 * sum_l T_l^2 elements; level l is the (T_l, T_l, 3) row-major block at
 * offset 3 * sum_{k<l} T_k^2.  L >= 2 needs T divisible by 2^(L-1) and T_{L-1} >= 2; L = 1 is a copy; T <= 16384, L <= 16.
 *   synth:   acc_{L-1} = level_{L-1}; acc_l = level_l + up2(acc_{l+1}); texture = acc_0, with up2 = F.interpolate(
 *            scale_factor=2, mode='bilinear', align_corners=False): fine 2j = 0.25 c[j-1] + 0.75 c[j], fine 2j+1 =
 *            0.75 c[j] + 0.25 c[j+1], indices clamped.  One launch whatever L is.
 *   adjoint: g_0 = grad_texture; g_{l+1} = up2^T(g_l); block l of grad_params = g_l -- every coarse texel gathers its
 *            <= 4 x 4 fine footprint in a fixed order (no atomics: bitwise reproducible).  At most two launches.
 * NaN / Inf propagate as the expressions say (taps that do not exist are skipped, never multiplied by zero).  The two
 * buffers of a call must not overlap.  Nothing is allocated.  st3d_texpyr_numel returns 0 for a shape the others refuse. */
size_t st3d_texpyr_numel(int T, int L);
int st3d_texpyr_synth(const float *params, int T, int L, float *texture, st3d_stream_t stream);
int st3d_texpyr_adjoint(const float *grad_texture, int T, int L, float *grad_params, st3d_stream_t stream);

/* ------------------------------------------------------------------ mip-mapped trilinear sampling (csrc/mipmap.hip,
 * DESIGN 7), hard settings, K = 1, unlit.  The chain lives in the texture pyramid's packed layout and has its limits
 * (T_l = T >> l; level l at float offset 3 * sum_{k<l} T_k^2; L >= 2 needs T divisible by 2^(L-1) and T_{L-1} >= 2;
 * T <= 16384, L <= 16); st3d_mip_numel returns 0 for a shape the others refuse.
 *   build:   level_0 = texture; level_{l+1}[r][x] = ((a + b) + (c + d)) * 0.25f over a = level_l[2r][2x], b = [2r][2x+1],
 *            c = [2r+1][2x], d = [2r+1][2x+1].  One launch, two for L > 6.
 *   adjoint: acc_{L-1} = g_{L-1}; acc_l[r][x] = g_l[r][x] + 0.25f * acc_{l+1}[r>>1][x>>1]; grad_texture = acc_0, added to
 *            what grad_texture holds when `accumulate`.  A gather in a fixed order, no atomics, one launch.
 *   lod:     lod (B,S,S): lambda = clamp(log2 rho + bias, 0, L-1) of every covered pixel from its fragment (face,
 *            barycentrics, zbuf) and the face's projected vertices (verts_ndc (B,V,3): x_ndc, y_ndc, view depth): rho is the
 *            larger of the lengths of d(u,v)/dx and d(u,v)/dy, times (T-1) texels and 2/S per pixel step.  0 where
 *            !(rho > 1), where the face's screen area is 0 and on uncovered pixels.  No neighbouring pixel is read.
 *   shade_mip_fwd: st3d_shade_fwd with texel = (1 - t) bil(l0) + t bil(l0 + 1), l0 = floor(lambda), t = lambda - l0; level
 *            l >= 1 is tapped at (ix + 0.5) / 2^l - 0.5 of the clamped level-0 index, clamped to its side.  t == 0 reads
 *            one level: lambda == 0 everywhere is st3d_shade_fwd bit for bit.
 *   shade_mip_bwd: lambda is a constant.  The texel gradients of both levels are scattered into grad_pyramid
 *            (st3d_mip_numel floats of the caller's, OVERWRITTEN; required iff grad_texture is given) and folded by the
 *            adjoint INTO grad_texture (accumulated).  workspace == NULL: float atomics; else the 64-bit fixed-point
 *            scatter (bitwise reproducible; a NaN / Inf in grad_rgb makes every element NaN), workspace of
 *            st3d_shade_mip_bwd_workspace_bytes(T, L) bytes, 16-byte aligned.  grad_uv (B,S,S,2), grad_bary (B,S,S,3) as
 *            st3d_shade_bwd, through both levels' taps.  Nothing is allocated. */
size_t st3d_mip_numel(int T, int L);
int st3d_mip_build(const float *texture, int T, int L, float *pyramid, st3d_stream_t stream);
int st3d_mip_adjoint(const float *grad_pyramid, int T, int L, int accumulate, float *grad_texture, st3d_stream_t stream);
int st3d_mip_lod(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *verts_ndc,
                 const int32_t *faces, const float *verts_uvs, const int32_t *faces_uvs, int B, int S, int T, int L, int V,
                 int F, int VT, float bias, float *lod, st3d_stream_t stream);
int st3d_shade_mip_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                       const float *verts_uvs, const int32_t *faces_uvs, const float *pyramid, const float *lod, int B, int S,
                       int T, int L, int F, int VT, float *rgb, float *mask, st3d_stream_t stream);
size_t st3d_shade_mip_bwd_workspace_bytes(int T, int L);
int st3d_shade_mip_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                       const float *dists, const float *verts_uvs, const int32_t *faces_uvs, const float *pyramid,
                       const float *lod, int B, int S, int T, int L, int F, int VT, float *grad_pyramid, float *grad_texture,
                       float *grad_uv, float *grad_bary, void *workspace, size_t workspace_bytes, st3d_stream_t stream);

/* ------------------------------------------------------------------ per-vertex colours (csrc/vcolor.hip):
 * PyTorch3D TexturesVertex on the hard settings (K = 1, blur 0, default BlendParams), unlit.  verts_colors (V,3) fp32 is
 * indexed by the mesh's own faces (F,3); there is no second index array.  Indices are NOT checked on the device: the
 * caller guarantees 0 <= faces < V and pix_to_face < F.
 *   shade_vc_fwd  replaces TexturesVertex.sample_textures (interpolate_face_attributes) + the ambient SoftPhongShader +
 *            softmax_rgb_blend: t_c = b0 C[v0][c] + b1 C[v1][c] + b2 C[v2][c] (left to right, uncontracted),
 *            rgb_c = (wnum t_c + delta) / denom with the blend and the mask of the UV forward; pixels without a face are
 *            white with mask 0.  rgb (B,3,S,S), mask (B,1,S,S).
 *   shade_vc_bwd  replaces the autograd backward of interpolate_face_attributes: with gk_c = grad_rgb_c wnum / denom,
 *            grad_colors[v_i][c] += b_i gk_c (float atomics; ACCUMULATED into grad_colors (V,3)) and grad_bary (B,S,S,3)
 *            = sum_c gk_c C[v_i][c], 0 on uncovered pixels, the input of st3d_raster_bwd.  Either output may be NULL, not
 *            both; without grad_colors nothing is scattered.
 *   shade_vc_bwd_det  the same with the scatter in 64-bit fixed point (bitwise reproducible; a NaN / Inf in grad_rgb,
 *            on a covered pixel or not, makes every element of grad_colors NaN; finite values on uncovered pixels change no
 *            bit).  grad_colors is required; workspace of st3d_shade_vc_bwd_det_workspace_bytes(V) bytes, 16-byte aligned.
 * S <= 4096.  Nothing is allocated. */
int st3d_shade_vc_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                      const int32_t *faces, const float *verts_colors, int B, int S, int F, int V, float *rgb, float *mask,
                      st3d_stream_t stream);
int st3d_shade_vc_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                      const float *dists, const int32_t *faces, const float *verts_colors, int B, int S, int F, int V,
                      float *grad_colors, float *grad_bary, st3d_stream_t stream);
size_t st3d_shade_vc_bwd_det_workspace_bytes(int V);
int st3d_shade_vc_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                          const float *dists, const int32_t *faces, const float *verts_colors, int B, int S, int F, int V,
                          float *grad_colors, float *grad_bary, void *workspace, size_t workspace_bytes,
                          st3d_stream_t stream);

/* ------------------------------------------------------------------ per-face texel atlas (csrc/atlas.hip):
 * PyTorch3D TexturesAtlas on the hard settings (K = 1, blur 0, default BlendParams), unlit.  atlas (F,R,R,3) fp32, 1 <= R
 * <= 64, F R^2 <= 2^31 - 1; every face owns an R x R block of texels addressed by the fragment's barycentrics.  Face
 * indices are NOT checked on the device: the caller guarantees pix_to_face < F.
 *   atlas_texel_index  host only, no GPU: the row wy and column wx of the texel of barycentrics (b0, b1) -- the function
 *            the kernels call (csrc/atlas.h): t_i = clamp(b_i R, 0, R - 1) in float (NaN -> 0), wx = (int)t0, wy = (int)t1,
 *            and (R-1-wx, R-1-wy) instead when (b0 + b1) R - (wx + wy) > 1.  Always within [0, R-1].
 *   shade_atlas_fwd  replaces TexturesAtlas.sample_textures + the ambient SoftPhongShader + softmax_rgb_blend:
 *            rgb_c = (wnum atlas[f][wy][wx][c] + delta) / denom with the blend and the mask of the UV forward; pixels
 *            without a face are white with mask 0.  rgb (B,3,S,S), mask (B,1,S,S).
 *   shade_atlas_bwd  its autograd backward: grad_atlas[f][wy][wx][c] += grad_rgb_c wnum / denom, one deposit per covered
 *            pixel (float atomics; ACCUMULATED into grad_atlas (F,R,R,3)).  The lookup is piecewise constant: there is no
 *            gradient towards the barycentrics.
 *   shade_atlas_bwd_det  the same with the scatter in 64-bit fixed point (bitwise reproducible; a NaN / Inf in grad_rgb,
 *            on a covered pixel or not, makes every element of grad_atlas NaN; finite values on uncovered pixels change no
 *            bit).  Workspace of st3d_shade_atlas_bwd_det_workspace_bytes(F, R) bytes (0 for arguments out of range),
 *            16-byte aligned.
 * S <= 4096.  Nothing is allocated. */
int st3d_atlas_texel_index(float b0, float b1, int R, int *wy, int *wx);
int st3d_shade_atlas_fwd(const int32_t *pix_to_face, const float *bary, const float *zbuf, const float *dists,
                         const float *atlas, int B, int S, int F, int R, float *rgb, float *mask, st3d_stream_t stream);
int st3d_shade_atlas_bwd(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                         const float *dists, int B, int S, int F, int R, float *grad_atlas, st3d_stream_t stream);
size_t st3d_shade_atlas_bwd_det_workspace_bytes(int F, int R);
int st3d_shade_atlas_bwd_det(const float *grad_rgb, const int32_t *pix_to_face, const float *bary, const float *zbuf,
                             const float *dists, int B, int S, int F, int R, float *grad_atlas, void *workspace,
                             size_t workspace_bytes, st3d_stream_t stream);

/* ------------------------------------------------------------------ optimiser:
 * torch.optim.Adam defaults (utils.py:185-195, style_transfer.py:57) */
int st3d_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                   int step, float lr, float beta1, float beta2, float eps, st3d_stream_t stream);

/* ------------------------------------------------------------------ fused perceptual engine:
 * losses.py:12-44 (compute_perceptual_loss) and the loop body of style_transfer.py:59-83.
 * One object per (VGG weights); one plan per (batch, image size). */
typedef struct st3d_vgg st3d_vgg;
typedef struct st3d_plan st3d_plan;

int st3d_vgg_create(st3d_vgg **out);
/* module_idx in torchvision's vgg19().features numbering (0,2,5,7,...,34); w (Cout,Cin,3,3), b (Cout) */
int st3d_vgg_set_conv(st3d_vgg *vgg, int module_idx, const float *w, const float *b,
                      st3d_stream_t stream);
int st3d_vgg_destroy(st3d_vgg *vgg);

/* workspace for batches of up to B images of S x S (any S >= 16; sizes off the fast path -- odd intermediate
 * resolutions, W % 4 != 0 -- run on the direct conv / separate pool kernels, pools floor like MaxPool2d) */
int st3d_plan_create(st3d_plan **out, st3d_vgg *vgg, int B, int S);
int st3d_plan_destroy(st3d_plan *plan);
size_t st3d_plan_bytes(const st3d_plan *plan);
/* forward of imgs (n,3,S,S), n <= B, through modules 0..upto_module (post-ReLU taps) */
int st3d_plan_forward(st3d_plan *plan, const float *imgs, int n, int upto_module, st3d_stream_t stream);
/* device pointer + shape of the activation after module_idx (a conv index = its post-ReLU
 * output, a pool index = the pooled output) of the last st3d_plan_forward */
int st3d_plan_activation(st3d_plan *plan, int module_idx, float **ptr, int *C, int *H, int *W);
/* targets (losses.py:18-25): conv4_2 features of content (B,3,S,S); Grams of style
 * (style_batch == 1: one image broadcast over the batch, as second_approach.py:157 repeats it) */
int st3d_plan_set_content(st3d_plan *plan, const float *content, int n, st3d_stream_t stream);
/* the content target (conv4_2 features, n x 512 x S/8 x S/8 floats) out of / into the plan: a caller alternating between
 * several view batches (second_approach.py:145-160 with n_views > batch_size) can keep each batch's target instead of
 * recomputing it every step */
int st3d_plan_get_content_features(st3d_plan *plan, float *out, int n, st3d_stream_t stream);
int st3d_plan_set_content_features(st3d_plan *plan, const float *features, int n, st3d_stream_t stream);
int st3d_plan_set_style(st3d_plan *plan, const float *style, int style_batch, int n, st3d_stream_t stream);
/* Guidance of the style term (default off): mask (n,1,S,S) fp32 in [0,1], NULL clears.  Builds the guidance planes
 * (st3d_guidance_build) into buffers the plan owns -- allocated by the first call that sets a guidance, st3d_plan_bytes
 * grows by st3d_guidance_floats(B, S) + B S^2 (w_0 = q_0^2 for the fused bottom pass) + 5 B + st3d_guidance_partials(B, S)
 * floats -- and every later st3d_plan_loss* call with the same n takes the Gram of each style tap over the guided region:
 * G^_l = sum_p w_l[p] F[:,p] F[:,p]^T in place of G_l, the gradient coef_l q o (D_l (q o F)).  The style targets stay the
 * plain Grams of the style image, the content term is unchanged, the guidance carries no gradient.  A loss call with
 * another n: ST3D_E_STATE.  Need masks, flat colours and graph replay work as without guidance (the planes' addresses
 * never change; a captured step is keyed on whether a guidance is set).  st3d_plan_forward / _backward are unaffected.
 * An image whose Sigma_l is 0 has G^_l = 0: its term is the constant ||S_l||^2 norm, with no gradient. */
int st3d_plan_set_style_guidance(st3d_plan *plan, const float *mask, int n, st3d_stream_t stream);
/* loss (losses.py:28-42) of current (n,3,S,S) and, if grad_current != NULL, d loss/d current.
 * batch_denom = the batch size the means divide by (n, or the GLOBAL batch when views are
 * sharded over ranks).  loss_out: device float[3] = {total, content_loss, style_loss}. */
int st3d_plan_loss(st3d_plan *plan, const float *current, int n, int batch_denom, float style_weight,
                   float content_weight, float *loss_out, float *grad_current, st3d_stream_t stream);
/* st3d_plan_loss for a caller whose only consumer of grad_current reads it at the pixels of need_mask (n,S,S bytes,
 * non-zero = read; 16-byte aligned; NULL = st3d_plan_loss): loss_out is bitwise st3d_plan_loss's; grad_current is bitwise
 * st3d_plan_loss's at those pixels and exactly 0 elsewhere.  The bottom launches of the backward then compute only what
 * those pixels need (st3d_need_blocks_build; ST3D_NEED_BLOCKS=0: st3d_need_build): the relu1_1 pass, the conv1_2 and the
 * conv2_1 input gradient and, where the full launch walks two tiles or more per workgroup, the relu2_1 Gram backward and the
 * conv2_2 .. conv3_3 input gradients -- ST3D_NEED_DEPTH = 0..7 masks fewer of them, bottom-up (A/B runs; 0 and sizes with
 * S % 64 != 0 run unmasked and return the full gradient).
 * With graph replay the mask is staged into a plan-owned buffer like the other inputs and the lists are built inside
 * the graph. */
int st3d_plan_loss_masked(st3d_plan *plan, const float *current, int n, int batch_denom, float style_weight,
                          float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask,
                          st3d_stream_t stream);
/* st3d_plan_loss_masked for a `current` that holds flat_color (3 floats in DEVICE memory; NULL = st3d_plan_loss_masked)
 * at many pixels, as a render holds its background: the forward launches of conv1_2, conv2_1 and conv2_2 compute the tiles
 * that see anything else plus one tile per border class of the rest, and the rest are copied (st3d_flat_build /
 * st3d_wino43_fwd_tiles / st3d_flat_fill).  Every activation, the losses and the gradient are bitwise what the call without
 * the colour gives: the device compares the pixels, the colour is a hint that costs the list build when it is wrong.
 * ST3D_FLAT=0 (read by every call) ignores the colour; ST3D_FLAT_DEPTH = 0..3 (read by st3d_plan_create) lists only the
 * first k of the three launches.  Sizes with S % 64 != 0 take the full path.  With graph replay the colour is staged and
 * the lists are built inside the graph. */
int st3d_plan_loss_flat(st3d_plan *plan, const float *current, int n, int batch_denom, float style_weight,
                        float content_weight, float *loss_out, float *grad_current, const uint8_t *need_mask,
                        const float *flat_color, st3d_stream_t stream);
/* st3d_plan_loss_flat for views whose geometry stays put while their texture changes.  epoch names a geometry epoch: the
 * caller promises that `cover` (n,S,S bytes, non-zero = covered; 16-byte aligned; it doubles as the need mask) has the
 * contents it had at every earlier call with this epoch and n, and -- when flat_color is given -- that every uncovered
 * pixel of `current` holds that colour bit for bit.  flat_rgb: the colour once more, 3 floats in HOST memory.  The plan then
 *   - keeps the need lists and the flat-field lists (built from cover: st3d_flat_build_cover) of the last three epochs and
 *     builds them only for an epoch it does not hold;
 *   - leaves out the three st3d_flat_fill launches while the buffers they write still hold this epoch's background: the
 *     previous call that wrote them was a keyed one with the same epoch, n, colour and weights.  Every other writer
 *     (st3d_plan_forward, st3d_plan_set_content, st3d_plan_set_style, any other st3d_plan_loss* call, a failed call,
 *     st3d_vgg_set_conv) makes the next keyed call fill again;
 *   - under the same condition runs conv1_1 over the tiles that see a covered pixel only (st3d_conv3x3_fwd_skip;
 *     ST3D_FLAT_CONV1=0, read by st3d_plan_create: the full launch);
 *   - under the same condition runs conv3_1, conv3_2 and conv3_3 over their kept lists (st3d_kept_build, built by the first
 *     such call of an epoch; st3d_wino43_fwd_strips): a tile the coverage cannot reach still holds the bits the previous call
 *     wrote, which the same launch on the same input would write again.  The first call of an epoch, and the first after any
 *     of the writers above, runs them in full.  Only where the full launch walks two tiles or more per workgroup.
 *     ST3D_KEEP_DEPTH = 0..3 (read by st3d_plan_create) lists fewer of them, bottom-up, 0 none; ST3D_KEEP_TILE = 64 | 32 | 16
 *     (or one value per launch, comma-separated): the geometry, default 16 = strips; ST3D_KEEP_FORCE=1 lifts the two-tiles
 *     rule (tests).
 *     In the same calls conv1_2, conv2_1 and conv2_2 walk their kept lists too instead of their flat-field lists, which have to
 *     name one tile per border class for the fills and are tied to the kernel's own geometry: ST3D_KEEP_SHALLOW = a,b,c, the
 *     geometry of each (64 | 32, 16 for conv2_1 only, 0 = the flat-field list as before; default 32,16,32).
 * Every activation, the losses and the gradient are bitwise st3d_plan_loss_flat's.  epoch == 0, cover == NULL or graph
 * replay on: st3d_plan_loss_flat itself, launch for launch.  ST3D_FLAT_CHECK=1 (read by st3d_plan_create): every keyed call
 * tests the promise about the uncovered pixels (st3d_flat_check_cover, one host read) and fails with ST3D_E_STATE if it
 * does not hold. */
int st3d_plan_loss_keyed(st3d_plan *plan, const float *current, int n, int batch_denom, float style_weight,
                         float content_weight, float *loss_out, float *grad_current, const uint8_t *cover,
                         const float *flat_color, const float *flat_rgb, uint64_t epoch, st3d_stream_t stream);
/* The split batch (ST3D_SPLIT_BATCH = 0 | 1 | fwd | bwd, read by st3d_plan_create; default fwd): a keyed call that finds the
 * clean record its own, with n even and at least 4, no guidance, no graph replay and profiling off, runs its images as two
 * groups of n / 2, the first on the caller's stream and the second on a stream of the plan's -- the forward to conv5_1, then
 * the Grams and the loss sums over the whole batch on the caller's stream, then the backward (fwd / bwd: that direction
 * alone, the other as one launch sequence; 1: both).  The plan's stream is forked
 * from the caller's stream and joined back to it by events before the call returns, so the caller orders its work as ever;
 * results are bitwise the one-stream call's.
 * st3d_plan_split_calls: how many calls so far ran their forward / their backward that way (either pointer may be NULL). */
int st3d_plan_split_calls(const st3d_plan *plan, int *forward_calls, int *backward_calls);
/* HIP-graph replay of st3d_plan_loss: its ~70 launches form a static sequence, so after one ordinary call it is captured
 * (per n / batch_denom / weights) and replayed with one hipGraphLaunch; inputs and outputs pass through plan-owned staging
 * buffers (three extra device copies per call).  Pays off where the step is launch-bound (small images). */
int st3d_plan_graph(st3d_plan *plan, int enable);
/* Backward of st3d_plan_forward for losses computed OUTSIDE the library on its taps (the reference's own loop body,
 * style_transfer.py:61-83, calls get_features(optimized_imgs) with grad and back-propagates through it):
 * grad_modules = host array of 37 device pointers, entry m = d loss / d (output of VGG module m) shaped like
 * st3d_plan_activation(m) for the n images of the last forward (NULL = none; a conv and the in-place ReLU behind it
 * are one tensor) -> grad_image (n,3,S,S). */
int st3d_plan_backward(st3d_plan *plan, int n, int upto_module, const float *const *grad_modules, float *grad_image,
                       st3d_stream_t stream);
/* per-kernel-family timing of the next calls (HIP events on the call's stream): enable, then
 * read accumulated milliseconds + launch counts; families: 0 conv_fwd (Winograd launches) 1 conv_dgrad (Winograd)
 * 2 pool 3 gram_fwd 4 gram_bwd 5 loss/elementwise 6 convx_fwd (convs Winograd does not cover: conv1_1, odd shapes)
 * 7 convx_dgrad 8 conv43_fwd 9 conv43_dgrad (Winograd F(4x4,3x3)); launches that ran over a need list
 * (st3d_plan_loss_masked) count under families of their own, their work being a fraction of the full launch's:
 * 10 conv43_dgrad_need 11 convx_dgrad_need (the relu1_1 pass) 12 gram_bwd_need (none yet); likewise the forward launches
 * over a flat-field list (st3d_plan_loss_flat) and the copies behind them: 13 conv43_fwd_flat 14 flat_fill; and the
 * conv1_1 launch that leaves out its background tiles (st3d_plan_loss_keyed): 15 convx_fwd_flat */
#define ST3D_PROFILE_FAMILIES 16
int st3d_plan_profile(st3d_plan *plan, int enable);
int st3d_plan_profile_read(st3d_plan *plan, float *ms_out /*host [ST3D_PROFILE_FAMILIES]*/,
                           int *launches_out /*host [ST3D_PROFILE_FAMILIES]*/);
/* Per-launch records gathered while profiling was on, since the previous call: tag = family * 100 + the VGG module
 * index the launch belongs to (99 = none), HIP-event milliseconds.  *count_out = records available; they are consumed
 * when `capacity` holds them all. */
int st3d_plan_profile_launches(st3d_plan *plan, int *tags_out /*host [capacity]*/, float *ms_out /*host [capacity]*/,
                               int capacity, int *count_out);

/* ------------------------------------------------------------------ Laplacian-preconditioned vertex steps (diffuse.hip)
 * Nicolet, Jacobson, Jakob, "Large Steps in Inverse Rendering of Geometry" (2021): the vertices are v = M^-1 u with
 * M = I + lambda L, L the combinatorial Laplacian of the static topology, (L x)_i = sum over j in nbr(i) of (x_i - x_j),
 * accumulated in exactly this form in adjacency order (nbr_off (V+1) / nbr_idx: the CSR adjacency, every index in [0, V) --
 * the CALLER guarantees it), so that M c = c bit for bit for a constant c.  M is symmetric positive definite, lambda_min >= 1.
 * st3d_diffuse_apply: y (V,3) = M x (V,3); x and y must not overlap.
 * st3d_diffuse_solve: x (V,3) = M^-1 b (V,3), the three columns by plain conjugate gradients from x = 0, each column in one
 * workgroup of 1024 threads with the whole iteration inside the kernel (no synchronisation between workgroups).  A column
 * stops when ||r||_2 <= tol ||b||_2 on the recursive residual or after max_iter iterations, whichever comes first -- a NaN in
 * b runs to max_iter and returns NaN in that column alone; b = 0 gives x = 0 after 0 iterations.  Dot products: fp32
 * products added in fp64 in a fixed order; two calls give the same bits.  The search direction lives in LDS while
 * 4 V + 256 bytes fit 160 KiB, else in the workspace; x, r and A p live in registers while V <= 4096, else in x and the
 * workspace.  ST3D_DIFFUSE_LDS=0 puts the search direction, ST3D_DIFFUSE_REGS=0 the other three, in global memory whatever
 * V is (both read by every call); the result is the same bits in every case.  workspace: st3d_diffuse_workspace_bytes(V) bytes (0 for V < 1), 16-byte
 * aligned, written before it is read.  info: 3 records {int32 iterations, int32 converged, float ||r|| / ||b||} (36 bytes,
 * 4-byte aligned), written on the device.  b and x must not overlap. */
int st3d_diffuse_apply(const int *nbr_off, const int *nbr_idx, int V, float lambda, const float *x, float *y,
                       st3d_stream_t stream);
size_t st3d_diffuse_workspace_bytes(int V);
int st3d_diffuse_solve(const int *nbr_off, const int *nbr_idx, int V, float lambda, const float *b, float *x, float tol,
                       int max_iter, void *workspace, size_t workspace_bytes, void *info, st3d_stream_t stream);
/* Adam with ONE second-moment denominator for the whole tensor (the update the paper above runs on u):
 *   m <- m + (g - m)(1 - beta1);  s <- beta2 s + (1 - beta2) g^2;
 *   p <- p - lr (m / (1 - beta1^t)) / (eps + max over all elements of sqrt(s / (1 - beta2^t)))
 * The maximum is order-free, so the result is the same bits from run to run; a NaN moment makes it NaN.  Two launches.
 * partials: st3d_reduce_partials() floats of scratch, written before they are read. */
int st3d_adam_step_uniform(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n, int step, float lr,
                           float beta1, float beta2, float eps, float *partials, st3d_stream_t stream);

/* ------------------------------------------------------------------ coverage-driven view selection (cover.hip)
 * Which texels of a T x T texture map each view touches, and a greedy choice of views by what each adds.  A mask is
 * W = (T*T + 31) / 32 32-bit words per view: texel (row r, column x) of the map as stored, (1,T,T,3) in original rows, has
 * index t = r*T + x and is bit t & 31 of word t >> 5; bits at or above T*T are 0.  Integer work only: two calls give the same
 * bits.  Every argument is checked on the host before any launch (ST3D_E_INVALID, nothing launched); nothing is allocated.
 * Masks, covered and the workspace are 4-byte aligned (rows are read 16 bytes at a time when W % 4 == 0 and the bases allow).
 * st3d_cover_mark: the hard K = 1 fragments of st3d_raster_fwd at side S, 1 <= S <= 4096, 1 <= T <= 16384.  For every
 *   covered pixel the UV is interpolated as st3d_shade_fwd does and each of the four texels of its bilinear footprint that
 *   lies inside the map with both weights > 0 -- the texels st3d_shade_bwd of a positive gradient adds a non-zero weight to --
 *   is ORed into view b's row of masks (B x W); bits already set stay.  faces_uvs must index verts_uvs and pix_to_face must
 *   index faces_uvs: the CALLER guarantees it.
 * st3d_cover_greedy: n rounds enqueued on the stream with no host read in between, 1 <= n <= C <= 4096, 1 <= W <= 2^26.
 *   Round k: gain[c] = sum_w popcount(masks[c][w] & ~covered[w]) for every candidate not yet taken; picks[k] = the untaken
 *   candidate of the largest gain, the lowest index among equals, gains[k] = its gain; covered |= its row; it is taken and
 *   never picked again (when every remaining gain is 0 the pick is the lowest untaken index, gain 0).  covered (W words): in =
 *   the texels already counted as seen, out = their union with the picks; it must not overlap masks.  workspace:
 *   st3d_cover_workspace_bytes(C) bytes (C gains + C taken flags; 0 for C outside 1...4096), written before it is read.
 * st3d_cover_count: counts (T*T int32)[t] = how many of the C >= 1 rows have bit t set; W must be (T*T + 31) / 32. */
int st3d_cover_mark(const int32_t *pix_to_face, const float *bary, const float *verts_uvs, const int32_t *faces_uvs, int B,
                    int S, int T, void *masks /* B x W, ORed into */, st3d_stream_t stream);
size_t st3d_cover_workspace_bytes(int C);
int st3d_cover_greedy(const void *masks /* C x W */, int C, int W, int n, void *covered /* W */, int32_t *picks /* n */,
                      int32_t *gains /* n */, void *workspace, st3d_stream_t stream);
int st3d_cover_count(const void *masks /* C x W */, int C, int W, int T, int32_t *counts /* T*T */, st3d_stream_t stream);

/* ------------------------------------------------------------------ baking views into the texture map (bake.hip)
 * UV-space back-projection: walk the texels of a T x T map, find each one's point on the surface, project it into every
 * view, test that it is visible there, read the view's colour and blend the views by how squarely they see it.  Gathers
 * throughout, no float atomics: two calls give the same bits.  Every argument is checked on the host before any launch
 * (ST3D_E_INVALID, nothing launched); nothing is allocated.  2 <= T <= 16384.
 * st3d_bake_surface (once per mesh): texel (row r, column x) of the map as stored sits at (x, T-1-r) in texel units, UV x
 *   (T-1) -- the inverse of the shading kernels' footprint.  t2f (T*T)[t] = the face whose UV triangle has the smallest squared
 *   distance d2 to the texel (0 inside or on the triangle, either winding; triangles without area and faces whose corners do
 *   not index verts_uvs (VT rows) are skipped), the lowest face among equal d2, provided d2 <= pad^2, 0 <= pad <= 8; else -1.
 *   tbary (T*T*3) = the barycentrics of the triangle's closest point (the texel's own inside, clamped onto an edge outside),
 *   0 where t2f = -1.  workspace: st3d_bake_workspace_bytes(T) bytes (one 64-bit key per texel; 0 for T outside the range),
 *   8-byte aligned, written before it is read.  Three enqueues: a memset, the claims (integer atomicMin), the decode.
 * st3d_bake_views (one launch per batch of views): for every texel with 0 <= t2f < F and every view b in index order:
 *   P = sum_i tbary_i v_i, n = the face's unit normal; view-space position as st3d_project_verts forms it, rejected at zv <=
 *   0.5; pixel position ix = ((1 - x_ndc) S - 1) / 2 (iy likewise), nearest pixel (rint) rejected outside the image; visible
 *   iff that pixel shows a face g >= 0 and (g == t2f or |zv - zbuf| <= depth_tol zv); c = |n . normalize(C - P)|, C = -T R^T,
 *   rejected below min_cos; colour = bilinear over the four pixels floor / floor + 1 (indices clamped to the image), taps on
 *   uncovered pixels dropped and the rest renormalised; w = c^power.  mode ST3D_BAKE_MEAN: acc.rgb += w colour, acc.w += w;
 *   ST3D_BAKE_BEST: acc = (w colour, w) when w > acc.w.  acc (T*T*4) is read and written: zeros start a bake, an earlier
 *   result continues it.  Texels with t2f outside 0...F-1 are not touched.  images (B,3,S,S); pix_to_face, zbuf (B,S,S): the
 *   hard K = 1 fragments of st3d_raster_fwd for (R, T) at side S <= 4096.  faces must index verts (V rows; a face that does
 *   not is skipped).
 * st3d_bake_resolve: out (T*T*3) = acc.rgb / acc.w where acc.w > 0, fallback (T*T*3) elsewhere, bit for bit. */
#define ST3D_BAKE_MEAN 0
#define ST3D_BAKE_BEST 1
size_t st3d_bake_workspace_bytes(int T);
int st3d_bake_surface(const float *verts_uvs, const int32_t *faces_uvs, int VT, int F, int T, float pad, void *workspace,
                      size_t workspace_bytes, int32_t *t2f, float *tbary, st3d_stream_t stream);
int st3d_bake_views(const float *verts, const int32_t *faces, int V, int F, const int32_t *t2f, const float *tbary, int Tt,
                    const float *R, const float *T, const float *images, const int32_t *pix_to_face, const float *zbuf, int B,
                    int S, float inv_tan_half_fov, int mode, float power, float min_cos, float depth_tol, float *acc,
                    st3d_stream_t stream);
int st3d_bake_resolve(const float *acc, const float *fallback, int Tt, float *out, st3d_stream_t stream);

/* ------------------------------------------------------------------ pull-push fill of a texture map (fill.hip)
 * Every texel of tex (H*W*3) that is not valid (H*W bytes, non-zero = valid) takes a colour interpolated from the valid
 * ones (Gortler et al. 1996), 1 <= H, W <= 16384.  A gather with fixed-order sums, an integer atomicAdd per wave for the
 * count and no float atomic: two calls give the same bits.  Every argument is checked on the host before any launch
 * (ST3D_E_INVALID, nothing launched); nothing is allocated.
 *   Level 0: w = valid ? 1 : 0, c = valid ? tex : 0 -- a select, never a product: what an invalid texel holds (NaN
 *     included) reaches no output.
 *   Pull: level l + 1 has sides ceil(h / 2), ceil(w / 2), down to 1 x 1.  Coarse texel (y, x) takes the children
 *     (2y + dy, 2x + dx) that exist, in the order (0,0), (0,1), (1,0), (1,1): W = sum w, C = sum w c; it stores c' = C / W
 *     where W > 0, else 0, and w' = min(W, 1).
 *   No valid texel anywhere (the 1 x 1 level has w = 0): out = tex bit for bit, count = 0, no error.
 *   Push, from the coarsest level to the finest: a texel with w >= 1 keeps its colour, any other takes w c + (1 - w) up, up
 *     = the 2x bilinear upsample of the completed coarser level at the texel's centre: along an axis the taps for index i
 *     are i/2 - 1 (weight 1/4) and i/2 (3/4) for even i, (i-1)/2 (3/4) and (i+1)/2 (1/4) for odd i, indices clamped to the
 *     coarser level; the four products (wy wx) c are summed in the order (y0,x0), (y0,x1), (y1,x0), (y1,x1).
 *   out (H*W*3) = tex bit for bit where valid, or where domain (H*W bytes, NULL = every texel) is given and 0; the pushed
 *     level-0 colour elsewhere.  count (one device int64, 8-byte aligned) = the texels that took the pushed colour.
 *   (A sum of weights that are 0 or 1, cut at 1, is 0 or 1: with this level 0 every w is 0 or 1, the pull averages the
 *   children that know a colour and the push hands a texel without one the upsample alone.)
 * workspace: st3d_fill_workspace_bytes(H, W) bytes, 16-byte aligned, written before it is read: one (rgb, w) float4 per
 *   texel of every level above the map, 16 max(1, sum_{l >= 1} h_l w_l) bytes, about H W 16 / 3; 0 for sides outside the
 *   range.  out must not be tex.  With ST3D_FILL_TAIL=0 in the environment (read per call) every level is a launch of its
 *   own instead of the coarse levels sharing one workgroup; the results are the same bits. */
size_t st3d_fill_workspace_bytes(int H, int W);
int st3d_fill_pushpull(const float *tex, const uint8_t *valid, const uint8_t *domain, int H, int W, void *workspace,
                       size_t workspace_bytes, float *out, int64_t *count, st3d_stream_t stream);

/* ------------------------------------------------------------------ image pyramid step (imgpyr.hip)
 * N planes of H x W fp32 (H, W even, 2...32768) halved with the separable tent filter [1 3 3 1] / 8 -- for sides >= 4 the
 * filter of an anti-aliased bilinear resize by 1/2, centred on every 2 x 2 block.  Every argument is checked on the host
 * before any launch (null pointers, N <= 0, odd or < 2 sides: ST3D_E_INVALID, nothing launched); nothing is allocated; the
 * two buffers of a call must not be the same.
 *   fwd:  out (N,H/2,W/2).  Coarse (i, j) reads rows 2i-1 ... 2i+2 and columns 2j-1 ... 2j+2, indices clamped to the plane.
 *         Per row h = (x[-1] + x[2]) + 3 (x[0] + x[1]); over the four h the same; then * (1/64) -- these roundings, in
 *         this order, no contraction.  NaN / Inf reach exactly the outputs whose footprint holds them.
 *   bwd:  grad_in (N,H,W), set, never added to: the exact transpose as a gather.  Along an axis fine index y has the near
 *         coarse index y >> 1 (weight 3) and the far one (y odd: near + 1, else near - 1; weight 1); where the far one is
 *         off the plane the near weight is 4 (the clamp had doubled that border row).  A fine pixel sums (wy wx / 64) g
 *         over (near,near), (near,far), (far,near), (far,far) in (row, column), in that order, taps that do not exist
 *         skipped: at most 4 products and 3 sums.  No atomics: two calls give the same bits.
 *   need: uint8 planes (Bn,H,W) -> (Bn,H/2,W/2), 1 where any pixel of the coarse pixel's clamped 4 x 4 footprint is
 *         non-zero, else 0: every coarse pixel a needed fine pixel gathers from in bwd is needed.
 *   tile: the fine pixels one workgroup owns in fwd and bwd (16 x 128); halos cross tile borders there. */
int st3d_pyr_down_tile(int *tile_h, int *tile_w);
int st3d_pyr_down_fwd(const float *in, int N, int H, int W, float *out, st3d_stream_t stream);
int st3d_pyr_down_bwd(const float *grad_out, int N, int H, int W, float *grad_in, st3d_stream_t stream);
int st3d_pyr_down_need(const uint8_t *need_in, int Bn, int H, int W, uint8_t *need_out, st3d_stream_t stream);

/* ------------------------------------------------------------------ colour control (color.hip)
 * Gatys et al. 2017, section 5: the luminance the style terms may be restricted to, and the colour matching of the style
 * image.  Every image is planar (B,3,P) fp32, P = H W pixels per channel plane, any P >= 1 (an odd P leaves channel planes
 * off 16-byte boundaries: the kernels then take scalar accesses).  Every argument is checked on the host before any launch
 * (null pointers, B <= 0, P == 0, B > 65535: ST3D_E_INVALID, nothing launched); nothing is allocated; an output must not be
 * one of the inputs.  All of it is per pixel and in a fixed order: NaN and +-Inf stay in their own pixel, no atomics, two
 * calls give the same bits.  The arithmetic, with W = (0.299f, 0.587f, 0.114f) (Rec. 601) as fp32 constants and fmaf one
 * rounding (tests/_colorref.py restates it in numpy):
 *     Y(r, g, b) = fmaf(W2, b, fmaf(W1, g, W0 * r))
 *   luma_fwd:   out[b,c,p] = Y(x[b,:,p]) for c = 0, 1, 2 -- a grey image is three equal planes, as the VGG plan takes them.
 *   luma_bwd:   the exact transpose: s = (g0 + g1) + g2 in fp32, in that order, then out_c = W_c * s.
 *   luma_recombine:  d = Y(opt) - Y(orig), one fp32 subtraction, then out_c = orig_c + d.  (The inverse YIQ transform has
 *               (1,1,1) as the column that multiplies Y: a new Y under the old I and Q adds the same d to all three.)
 *   color_affine:    out_c = fmaf(A[c][2], x2, fmaf(A[c][1], x1, fmaf(A[c][0], x0, b_c))); with clamp != 0 then
 *               v < 0 ? 0 : (v > 1 ? 1 : v) -- a NaN stays a NaN, as in torch.clamp. 
 *               A9 (row-major 3 x 3) and b3 are fp32 in HOST memory, read during the call and handed to the kernel by
 *               value: no upload, nothing to keep alive.
 *   color_stats:     mask (B,P) bytes, NULL = every pixel.  out10 (10 doubles, device), over the pixels whose mask byte is
 *               non-zero: [0] the count, [1..3] sum x_c, [4..9] sum x_c x_d for (c,d) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).
 *               The products are formed in fp64 from the fp32 values (exact), the sums are fp64 in a fixed two-stage
 *               order: a workgroup of 256 threads owns st3d_color_stats_chunk() consecutive pixels of one image, thread
 *               t adds pixels t, t + 256, ... in ascending order, the 256 sums are folded by halving strides (128 ... 1);
 *               a second launch adds the partials in index order (image-major, then chunk).
 *               partials: 10 * B * ceil(P / chunk) doubles of scratch, written before they are read. */
int st3d_color_stats_chunk(void);
int st3d_luma_fwd(const float *x, int B, size_t P, float *out, st3d_stream_t stream);
int st3d_luma_bwd(const float *g, int B, size_t P, float *out, st3d_stream_t stream);
int st3d_luma_recombine(const float *opt, const float *orig, int B, size_t P, float *out, st3d_stream_t stream);
int st3d_color_affine(const float *x, const float *A9, const float *b3, int clamp, int B, size_t P, float *out,
                      st3d_stream_t stream);
int st3d_color_stats(const float *x, const uint8_t *mask, int B, size_t P, double *partials, double *out10,
                     st3d_stream_t stream);

/* ------------------------------------------------------------------ Laplacian content term (lap.hip)
 * Li, Xu, Nie and Chua 2017: the squared difference between the Laplacian of the average-pooled image and a target.  A
 * stack of N planes (H,W) fp32 (every channel on its own) and a pool side p in {1,2,4,8,16} that divides H and W, with
 * h = H/p >= 2, w = W/p >= 2 and sides <= 32768.  Every argument is checked on the host before any launch (null or aliased
 * pointers, bad sides, bad p, a grid that does not fit one dimension, a workspace too small: ST3D_E_INVALID, nothing
 * launched); nothing is allocated.  No atomics: two calls give the same bits.  The arithmetic, fp32 unless stated, nothing
 * fused (tests/_lapref.py restates it in numpy):
 *   pool:  s_r = ((x(ip+r, jp) + x(ip+r, jp+1)) + ...) + x(ip+r, jp+p-1) for the p rows of the block, left to right;
 *          P(i,j) = ((s_0 + s_1) + ... + s_{p-1}) * (1/p^2), top to bottom, one product with the exact constant.  p = 1: P = x.
 *   D:     L(i,j) = 4 P(i,j) - ((P(i-1,j) + P(i+1,j)) + (P(i,j-1) + P(i,j+1))), indices clamped to the plane.  D is symmetric.
 *   lap_fwd:  out (N,h,w) = D(pool_p(x)).
 *   lap_loss: r = D(pool_p(x)) - target, target (N,h,w);  loss[0] = fp32(scale * sum r^2), the squares and the sum in fp64:
 *          a workgroup of 256 threads owns one tile of st3d_lap_tile(p) fine pixels, i.e. (tile_h/p) x (tile_w/p) cells
 *          numbered row-major; thread t adds the cells t, t + 256, ... of the tile that lie on the plane in ascending
 *          order, the 256 sums are folded by halving strides (128 ... 1); workgroups are numbered plane-major, then tile row,
 *          then tile column; the finishing launch has thread t add the partials t, t + 256, ... and folds the same way.
 *          grad (N,H,W), or NULL for the value alone: grad(y,x) = k * D(r)(y/p, x/p), k = fp32(2 scale / p^2) formed on
 *          the host, one product per cell.  scale is finite and >= 0.
 *          workspace: st3d_lap_workspace_bytes(N,H,W,p) bytes of device scratch, 8-byte aligned, written before it is
 *          read (the partials, and r at pooled size).  Launches: 3 with grad, 2 without.
 *   st3d_lap_workspace_bytes: 0 for arguments the calls refuse. */
int st3d_lap_tile(int p, int *tile_h, int *tile_w);
size_t st3d_lap_workspace_bytes(int N, int H, int W, int p);
int st3d_lap_fwd(const float *x, int N, int H, int W, int p, float *out, st3d_stream_t stream);
int st3d_lap_loss(const float *x, const float *target, int N, int H, int W, int p, double scale, void *workspace,
                  size_t workspace_bytes, float *loss, float *grad, st3d_stream_t stream);

/* ------------------------------------------------------------------ multi-GPU
 * One process per GPU; every rank renders / VGGs its slice of the view batch with the loss means divided by the GLOBAL
 * batch (batch_denom of st3d_plan_loss) and ONE SUM all-reduce of the flat fp32 gradient (3*T*T texture floats
 * [+ 3*V vertex floats]) makes the gradients identical everywhere before the replicated st3d_adam_step.  The reference
 * has no multi-GPU path (no torch.distributed / NCCL call site anywhere); the Python host of this package goes through
 * torch.distributed (backend "nccl" = RCCL on ROCm) -- these entry points give a C caller the same collective: RCCL's
 * ncclAllReduce over xGMI, bound at run time (no link-time dependency).  Rank 0 creates the id and hands the 128 bytes to
 * the other ranks by any out-of-band means (file, env, socket); each rank then calls st3d_comm_init with its HIP
 * device current. */
#define ST3D_COMM_ID_BYTES 128
typedef struct st3d_comm st3d_comm;
int st3d_comm_unique_id(unsigned char id_out[ST3D_COMM_ID_BYTES]);
int st3d_comm_init(st3d_comm **out, int rank, int world, const unsigned char unique_id[ST3D_COMM_ID_BYTES]);
int st3d_allreduce_sum_f32(st3d_comm *comm, float *buf /* device, in place */, size_t n, st3d_stream_t stream);
int st3d_comm_destroy(st3d_comm *comm);

/* Named ranges for rocprofv3 --marker-trace (the reference's only progress reporting are tqdm bars,
 * style_transfer.py:59, first_approach.py:191, second_approach.py:145).  With ST3D_ROCTX=1 in the environment the library
 * binds libroctx64 at run time and st3d_plan_loss / st3d_plan_forward / st3d_plan_backward mark their phases (vgg_forward,
 * gram_and_losses, vgg_backward); hosts bracket their own phases with push / pop (the Python host: render, render_backward,
 * allreduce, adam).  Without it every call returns at once.  st3d_trace_enabled: 1 when ranges are being emitted. */
int st3d_trace_push(const char *name);
int st3d_trace_pop(void);
int st3d_trace_enabled(void);

#ifdef __cplusplus
}
#endif
#endif /* ST3D_H */
