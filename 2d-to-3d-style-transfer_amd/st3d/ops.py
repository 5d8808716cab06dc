"""Tensor-level wrappers over the C ABI (one function per include/st3d.h entry point).
PyTorch owns the device memory and the stream; every call goes to libst3d.so."""
import ctypes
import math
import os

import torch

from . import _lib
from ._lib import call, dptr, stream_ptr

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
INV_TAN_HALF_FOV = float(1.0 / math.tan(math.radians(60.0) / 2.0))   # FoVPerspectiveCameras default fov=60


def _f32c(t):
    return t.detach().to(F32).contiguous()


# The texture / vertex gradient scatters of the render backward -- the specialised K = 1 path and, since round 3, the
# general soft path -- accumulate in 64-bit fixed point (csrc/det.h): bitwise reproducible from run to run, and measured
# no slower than the float-atomic kernels (0.128 vs 0.137 ms for the texture scatter of config 2), so it is the default.  set_deterministic(False) / ST3D_DETERMINISTIC=0 selects the float atomics.
_DETERMINISTIC = os.environ.get("ST3D_DETERMINISTIC", "1") not in ("", "0")


def set_deterministic(on=True):
    global _DETERMINISTIC
    _DETERMINISTIC = bool(on)


def is_deterministic():
    return _DETERMINISTIC


# ------------------------------------------------------------------ render
def project_verts(verts, R, T):
    """verts (V,3), R (B,3,3), T (B,3) -> (B,V,3) (x_ndc, y_ndc, z_view)."""
    verts, R, T = _f32c(verts), _f32c(R), _f32c(T)
    B, V = R.shape[0], verts.shape[0]
    out = torch.empty((B, V, 3), dtype=F32, device=verts.device)
    call("st3d_project_verts", dptr(verts), V, dptr(R), dptr(T), B, INV_TAN_HALF_FOV, dptr(out), stream_ptr())
    return out


# ---- near-plane watch of the specialised K = 1 rasteriser.  PyTorch3D clips every mesh at z_clip_value = znear / 2 before
# rasterising; the K = 1 / blur 0 kernels do not clip (for the reference's cameras nothing comes nearer than 0.78), so they
# raise a device flag when a rasterised face has a vertex nearer than z_clip.  The flag travels to pinned host memory
# without blocking and is looked at when a later call finds its copy complete (or by check_near_plane(block=True)).
# Policy (ST3D_NEAR_PLANE, default "clip"): from then on every render of the process goes through the general kernels,
# which clip exactly like PyTorch3D (st3d.render.render_views asks near_plane_triggered()), with one warning.  "raise":
# fail loudly.  This asynchronous watch is the safety net of DIRECT raster_fwd callers: st3d.render.render_views asks
# reaches_near_plane() BEFORE it renders (round 3), so through the renderer no frame is ever rendered unclipped -- a vertex
# optimisation that drives the mesh into the near plane (bob, 'both', lr 0.01: after ~80 steps) moves to the clipping
# kernels with the first such frame and keeps running like the reference does.
_NEAR_PENDING = []
_NEAR_TRIGGERED = False
_NEAR_WARNED = False
NEAR_PLANE_POLICY = os.environ.get("ST3D_NEAR_PLANE", "clip")
NEAR_PLANE_MESSAGE = ("a rasterised face has a vertex nearer than z_clip_value (PyTorch3D clips meshes at znear / 2 = 0.5); the "
                      "specialised K = 1 kernels do not clip -- construct RasterizationSettings(z_clip_value=0.5) to render "
                      "through the general kernels, which do")


def near_plane_triggered():
    return _NEAR_TRIGGERED


def reset_near_plane():
    global _NEAR_TRIGGERED, _NEAR_WARNED
    _NEAR_TRIGGERED = _NEAR_WARNED = False
    _NEAR_PENDING.clear()


def note_near_plane():
    """One warning per process the first time a render is sent to the clipping kernels."""
    global _NEAR_WARNED
    if not _NEAR_WARNED:
        import warnings
        warnings.warn("st3d: the mesh reached the near clipping plane (z < znear / 2); rendering continues on the general "
                      "kernels, which clip like PyTorch3D (ST3D_NEAR_PLANE=raise turns this into an error)")
        _NEAR_WARNED = True


def check_near_plane(block=False):
    global _NEAR_TRIGGERED
    while _NEAR_PENDING:
        host, ev = _NEAR_PENDING[0]
        if block:
            ev.synchronize()
        elif not ev.query():
            break
        _NEAR_PENDING.pop(0)
        if int(host[0]) != 0:
            _NEAR_PENDING.clear()
            if NEAR_PLANE_POLICY == "raise":
                raise RuntimeError(NEAR_PLANE_MESSAGE)
            note_near_plane()
            _NEAR_TRIGGERED = True


def raster_fwd(verts_ndc, faces_i32, S, z_clip=None):
    """-> pix_to_face (B,S,S) int32, zbuf (B,S,S), bary (B,S,S,3), dists (B,S,S).  z_clip: depth the near-plane watch
    compares with (None = no watch)."""
    B, V, _ = verts_ndc.shape
    F = faces_i32.shape[0]
    dev = verts_ndc.device
    ws_bytes = _lib.load().st3d_raster_workspace_bytes_binned(B, F, S)       # room for the coarse face bins too
    ws = torch.empty(((ws_bytes + 3) // 4,), dtype=F32, device=dev)
    p2f = torch.empty((B, S, S), dtype=I32, device=dev)
    zbuf = torch.empty((B, S, S), dtype=F32, device=dev)
    bary = torch.empty((B, S, S, 3), dtype=F32, device=dev)
    dists = torch.empty((B, S, S), dtype=F32, device=dev)
    flag = torch.zeros((1,), dtype=I32, device=dev) if z_clip is not None else None
    call("st3d_raster_fwd", dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, F, S, dptr(ws), ws_bytes, dptr(p2f),
         dptr(zbuf), dptr(bary), dptr(dists), float(z_clip or 0.0), dptr(flag), stream_ptr())
    if flag is not None:
        check_near_plane()
        host = torch.empty((1,), dtype=I32, pin_memory=True)
        host.copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _NEAR_PENDING.append((host, ev))
    return p2f, zbuf, bary, dists


# ---- what the renderer wrappers below share.  These build argument tuples and buffers and never launch: every public
# wrapper holds its own call("st3d_...") (the guarded suite finds the device wrappers by that text).
def _frag_head(frag):
    """the four fragment pointers in the order of the C ABI: p2f, bary, zbuf, dists"""
    p2f, zbuf, bary, dists = frag
    return dptr(p2f, I32), dptr(bary, F32), dptr(zbuf, F32), dptr(dists, F32)


def _uv_head(verts_uvs, faces_uvs_i32, texture):
    return dptr(verts_uvs, F32), dptr(faces_uvs_i32, I32), dptr(texture, F32)


def _rgb_mask(B, S, device):
    """the (rgb (B,3,S,S), mask (B,1,S,S)) pair every shade_*_fwd fills"""
    return torch.empty((B, 3, S, S), dtype=F32, device=device), torch.empty((B, 1, S, S), dtype=F32, device=device)


def _det_ws(nbytes, device):
    """-> (workspace of a fixed-point scatter, its size in bytes): whole 16-byte units, as floats"""
    return torch.empty(((nbytes + 15) // 16 * 4,), dtype=F32, device=device), nbytes


def _outputs(first, *optional):
    """first [, t for every (wanted, t) of optional that is wanted]; a lone output is returned bare"""
    out = (first,) + tuple(t for wanted, t in optional if wanted)
    return out if len(out) > 1 else out[0]


def shade_fwd(frag, verts_uvs, faces_uvs_i32, texture):
    B, S, _ = frag[0].shape
    rgb, mask = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, texture.shape[0],
         faces_uvs_i32.shape[0], verts_uvs.shape[0], dptr(rgb), dptr(mask), stream_ptr())
    return rgb, mask


def shade_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, grad_texture=None, want_uv=False, want_bary=False,
              want_texture=True):
    """-> grad_texture (T,T,3) [, grad_uv (B,S,S,2)] [, grad_bary (B,S,S,3)]"""
    B, S, _ = frag[0].shape
    T, dev = texture.shape[0], frag[0].device
    if grad_texture is None and want_texture:
        grad_texture = torch.zeros((T, T, 3), dtype=F32, device=dev)
    guv = torch.empty((B, S, S, 2), dtype=F32, device=dev) if want_uv else None
    gbary = torch.empty((B, S, S, 3), dtype=F32, device=dev) if want_bary else None
    grad_rgb = grad_rgb.contiguous()
    head = (dptr(grad_rgb, F32), *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, T,
            faces_uvs_i32.shape[0], verts_uvs.shape[0], dptr(grad_texture, F32), dptr(guv), dptr(gbary))
    if _DETERMINISTIC and grad_texture is not None:
        ws, nb = _det_ws(_lib.load().st3d_shade_bwd_det_workspace_bytes(T), dev)
        call("st3d_shade_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_shade_bwd", *head, stream_ptr())
    return _outputs(grad_texture, (want_uv, guv), (want_bary, gbary))


# ---- per-vertex colours (csrc/vcolor.hip): TexturesVertex on the hard settings, unlit
def _vc_check(p2f, faces_i32, colours):
    """the shapes the kernels index with: colours (V,3), faces (F,3); the CALLER guarantees faces < V (Meshes.faces_i32)"""
    if colours.dim() != 2 or colours.shape[1] != 3 or colours.shape[0] < 1:
        raise ValueError(f"vertex colours must be (V, 3), got {tuple(colours.shape)}")
    if faces_i32.dim() != 2 or faces_i32.shape[1] != 3 or faces_i32.shape[0] < 1:
        raise ValueError(f"faces must be (F, 3), got {tuple(faces_i32.shape)}")
    if p2f.dim() != 3 or p2f.shape[1] != p2f.shape[2]:
        raise ValueError(f"pix_to_face must be (B, S, S), got {tuple(p2f.shape)}")


def shade_vc_fwd(frag, faces_i32, colours):
    """frag, faces (F,3) int32, colours (V,3) -> rgb (B,3,S,S), mask (B,1,S,S)"""
    p2f = frag[0]
    _vc_check(p2f, faces_i32, colours)
    B, S, _ = p2f.shape
    rgb, mask = _rgb_mask(B, S, p2f.device)
    call("st3d_shade_vc_fwd", *_frag_head(frag), dptr(faces_i32, I32), dptr(colours, F32), B, S, faces_i32.shape[0],
         colours.shape[0], dptr(rgb), dptr(mask), stream_ptr())
    return rgb, mask


def shade_vc_bwd(grad_rgb, frag, faces_i32, colours, grad_colours=None, want_colours=True, want_bary=False):
    """-> grad_colours (V,3) (accumulated into `grad_colours` when given) [, grad_bary (B,S,S,3)]; want_colours=False
    (the vertices alone are optimised): grad_bary alone, nothing is scattered.  The scatter follows is_deterministic()."""
    p2f = frag[0]
    _vc_check(p2f, faces_i32, colours)
    B, S, _ = p2f.shape
    V, F = colours.shape[0], faces_i32.shape[0]
    if tuple(grad_rgb.shape) != (B, 3, S, S):
        raise ValueError(f"grad_rgb must be {(B, 3, S, S)}, got {tuple(grad_rgb.shape)}")
    if not (want_colours or want_bary):
        raise ValueError("shade_vc_bwd: nothing asked for (want_colours and want_bary are both False)")
    if not want_colours:
        grad_colours = None
    elif grad_colours is None:
        grad_colours = torch.zeros((V, 3), dtype=F32, device=p2f.device)
    gbary = torch.empty((B, S, S, 3), dtype=F32, device=p2f.device) if want_bary else None
    grad_rgb = grad_rgb.contiguous()
    head = (dptr(grad_rgb, F32), *_frag_head(frag), dptr(faces_i32, I32), dptr(colours, F32), B, S, F, V,
            dptr(grad_colours, F32), dptr(gbary))
    if _DETERMINISTIC and grad_colours is not None:
        ws, nb = _det_ws(_lib.load().st3d_shade_vc_bwd_det_workspace_bytes(V), p2f.device)
        call("st3d_shade_vc_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_shade_vc_bwd", *head, stream_ptr())
    if want_colours and want_bary:
        return grad_colours, gbary
    return grad_colours if want_colours else gbary


# ---- per-face texel atlas (csrc/atlas.hip): TexturesAtlas on the hard settings, unlit
ATLAS_MAX_R = 64


def _atlas_check(p2f, F, R):
    """the sizes the kernels index with; the CALLER guarantees pix_to_face < F (the fragments of a mesh of F faces)"""
    if not 1 <= R <= ATLAS_MAX_R:
        raise ValueError(f"atlas resolution R must be 1...{ATLAS_MAX_R}, got {R}")
    if F < 1 or F * R * R > 2 ** 31 - 1:
        raise ValueError(f"an atlas needs 1 <= F and F R^2 <= 2^31 - 1 (the tile table's keys are int), got F = {F}, R = {R}")
    if p2f.dim() != 3 or p2f.shape[1] != p2f.shape[2]:
        raise ValueError(f"pix_to_face must be (B, S, S), got {tuple(p2f.shape)}")


def shade_atlas_fwd(frag, atlas):
    """frag, atlas (F,R,R,3) -> rgb (B,3,S,S), mask (B,1,S,S)"""
    p2f = frag[0]
    if atlas.dim() != 4 or atlas.shape[3] != 3 or atlas.shape[1] != atlas.shape[2]:
        raise ValueError(f"atlas must be (F, R, R, 3), got {tuple(atlas.shape)}")
    F, R = atlas.shape[0], atlas.shape[1]
    _atlas_check(p2f, F, R)
    B, S, _ = p2f.shape
    rgb, mask = _rgb_mask(B, S, p2f.device)
    call("st3d_shade_atlas_fwd", *_frag_head(frag), dptr(atlas, F32), B, S, F, R, dptr(rgb), dptr(mask), stream_ptr())
    return rgb, mask


def shade_atlas_bwd(grad_rgb, frag, R, F, grad_atlas=None):
    """-> grad_atlas (F,R,R,3) (accumulated into `grad_atlas` when given).  The scatter follows is_deterministic()."""
    p2f = frag[0]
    R, F = int(R), int(F)
    _atlas_check(p2f, F, R)
    B, S, _ = p2f.shape
    if tuple(grad_rgb.shape) != (B, 3, S, S):
        raise ValueError(f"grad_rgb must be {(B, 3, S, S)}, got {tuple(grad_rgb.shape)}")
    if grad_atlas is None:
        grad_atlas = torch.zeros((F, R, R, 3), dtype=F32, device=p2f.device)
    elif tuple(grad_atlas.shape) != (F, R, R, 3):
        raise ValueError(f"grad_atlas must be {(F, R, R, 3)}, got {tuple(grad_atlas.shape)}")
    grad_rgb = grad_rgb.contiguous()
    head = (dptr(grad_rgb, F32), *_frag_head(frag), B, S, F, R, dptr(grad_atlas, F32))
    if _DETERMINISTIC:
        ws, nb = _det_ws(_lib.load().st3d_shade_atlas_bwd_det_workspace_bytes(F, R), p2f.device)
        call("st3d_shade_atlas_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_shade_atlas_bwd", *head, stream_ptr())
    return grad_atlas


# ---- supersampling (csrc/shade.hip): fragments at side a * S, images and their gradients at side S
MAX_RASTER_SIDE = 4096
SUPERSAMPLE_MAX = 4


def check_supersample(a, S=None):
    """a must be an int in 1..4 (ValueError) and a * S within the rasteriser's 4096."""
    if isinstance(a, bool) or not isinstance(a, int) or not 1 <= a <= SUPERSAMPLE_MAX:
        raise ValueError(f"supersample must be an int in 1..{SUPERSAMPLE_MAX}, got {a!r}")
    if S is not None and a * int(S) > MAX_RASTER_SIDE:
        raise ValueError(f"supersample * image_size = {a} * {S} exceeds the rasteriser's {MAX_RASTER_SIDE}")
    return a


def _ss_side(p2f, a):
    B, SS, _ = p2f.shape
    check_supersample(a)
    if SS % a:
        raise ValueError(f"fragments of side {SS} are no multiple of supersample = {a}")
    return B, SS // a


def box_down_fwd(x, a):
    """(B,C,a*S,a*S) -> (B,C,S,S): ordered row-major sum of every a x a block / a^2"""
    check_supersample(a)
    B, C, SS, W = x.shape
    if SS != W or SS % a:
        raise ValueError(f"box_down_fwd takes square images whose side is a multiple of {a}, got {tuple(x.shape)}")
    out = torch.empty((B, C, SS // a, SS // a), dtype=F32, device=x.device)
    call("st3d_box_down_fwd", dptr(x.contiguous(), F32), B, C, SS // a, a, dptr(out), stream_ptr())
    return out


def box_down_bwd(grad_out, a):
    """(B,C,S,S) -> (B,C,a*S,a*S): grad_out / a^2 at every sub-pixel"""
    check_supersample(a)
    B, C, S, W = grad_out.shape
    if S != W:
        raise ValueError(f"box_down_bwd takes square images, got {tuple(grad_out.shape)}")
    check_supersample(a, S)
    out = torch.empty((B, C, a * S, a * S), dtype=F32, device=grad_out.device)
    call("st3d_box_down_bwd", dptr(grad_out.contiguous(), F32), B, C, S, a, dptr(out), stream_ptr())
    return out


def shade_ss_fwd(frag, verts_uvs, faces_uvs_i32, texture, a):
    """frag at side a*S -> rgb (B,3,S,S), coverage (B,1,S,S) in {0, 1/a^2, ..., 1}"""
    B, S = _ss_side(frag[0], a)
    rgb, cov = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_ss_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, a, texture.shape[0],
         faces_uvs_i32.shape[0], verts_uvs.shape[0], dptr(rgb), dptr(cov), stream_ptr())
    return rgb, cov


def shade_ss_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, a, grad_texture=None, want_uv=False, want_bary=False,
                 want_texture=True):
    """grad_rgb (B,3,S,S), frag at side a*S -> grad_texture (T,T,3) [, grad_uv (B,aS,aS,2)] [, grad_bary (B,aS,aS,3)]"""
    B, S = _ss_side(frag[0], a)
    SS = a * S
    T, dev = texture.shape[0], frag[0].device
    if tuple(grad_rgb.shape) != (B, 3, S, S):
        raise ValueError(f"grad_rgb must be {(B, 3, S, S)}, got {tuple(grad_rgb.shape)}")
    if grad_texture is None and want_texture:
        grad_texture = torch.zeros((T, T, 3), dtype=F32, device=dev)
    guv = torch.empty((B, SS, SS, 2), dtype=F32, device=dev) if want_uv else None
    gbary = torch.empty((B, SS, SS, 3), dtype=F32, device=dev) if want_bary else None
    grad_rgb = grad_rgb.contiguous()
    head = (dptr(grad_rgb, F32), *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, a, T,
            faces_uvs_i32.shape[0], verts_uvs.shape[0], dptr(grad_texture, F32), dptr(guv), dptr(gbary))
    if _DETERMINISTIC and grad_texture is not None:
        ws, nb = _det_ws(_lib.load().st3d_shade_bwd_det_workspace_bytes(T), dev)
        call("st3d_shade_ss_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_shade_ss_bwd", *head, stream_ptr())
    return _outputs(grad_texture, (want_uv, guv), (want_bary, gbary))


def raster_bwd(grad_bary, p2f, verts_ndc, faces_i32):
    """grad_bary (B,S,S,3) -> grad_verts_ndc (B,V,3)"""
    B, V, _ = verts_ndc.shape
    S = p2f.shape[1]
    g = torch.empty((B, V, 3), dtype=F32, device=verts_ndc.device)
    head = (dptr(grad_bary, F32), dptr(p2f, I32), dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, faces_i32.shape[0], S,
            dptr(g))
    if _DETERMINISTIC:
        ws, nb = _det_ws(_lib.load().st3d_raster_bwd_det_workspace_bytes(B, V, S), verts_ndc.device)
        call("st3d_raster_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_raster_bwd", *head, stream_ptr())
    return g


def project_verts_bwd(verts, R, T, grad_ndc, out=None):
    verts, R, T = _f32c(verts), _f32c(R), _f32c(T)
    acc = 1
    if out is None:
        out = torch.empty_like(verts)
        acc = 0
    call("st3d_project_verts_bwd", dptr(verts), verts.shape[0], dptr(R), dptr(T), R.shape[0], INV_TAN_HALF_FOV,
         dptr(grad_ndc, F32), acc, dptr(out), stream_ptr())
    return out


def mesh_reg(verts, target, topo, weights, want_grad=True):
    """topo: dict(edges (E,2) i32, nbr_off (V+1) i32, nbr_idx i32, pairs (P,4) i32, pair_off (V+1) i32, pair_ref (4P) i32).
    -> (loss_out [weighted total, mse, edge, laplacian, normal], grad_verts (V,3) or None)"""
    verts, target = _f32c(verts), _f32c(target)
    V = verts.shape[0]
    dev = verts.device
    P = topo["pairs"].shape[0]
    scratch = torch.empty((_lib.load().st3d_mesh_reg_scratch_floats(V, P),), dtype=F32, device=dev)
    parts = torch.empty((4 * _lib.load().st3d_reduce_partials(),), dtype=F32, device=dev)
    out = torch.zeros((5,), dtype=F32, device=dev)
    g = torch.zeros_like(verts) if want_grad else None
    w = (ctypes.c_float * 4)(*[float(x) for x in weights])
    call("st3d_mesh_reg", dptr(verts), dptr(target), V, dptr(topo["edges"], I32), topo["edges"].shape[0],
         dptr(topo["nbr_off"], I32), dptr(topo["nbr_idx"], I32), dptr(topo["pairs"], I32) if P else None, P,
         dptr(topo["pair_off"], I32) if P else None, dptr(topo["pair_ref"], I32) if P else None, w,
         dptr(scratch), dptr(parts), dptr(out), dptr(g), stream_ptr())
    return out, g


LAPLACIAN_METHODS = {"uniform": 0, "cot": 1, "cotcurv": 2}


def check_edge_target_length(t):
    """a finite float >= 0; else ValueError"""
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not (math.isfinite(t) and t >= 0.0):
        raise ValueError(f"target_length must be a finite number >= 0, got {t!r}")
    return float(t)


def mesh_reg_ex(verts, target, topo, cot_topo, weights, laplacian_method="uniform", edge_target_length=0.0, want_grad=True):
    """mesh_reg with the Laplacian of `laplacian_method` ('uniform' | 'cot' | 'cotcurv') and an edge target length >= 0.
    cot_topo: mesh_losses.build_cot_topology's dict (faces (F,3), nbr_edge (2E), edge_off (E+1), edge_ref (3F), inc_off (V+1),
    inc_ref (3F), all i32); may be None for 'uniform'.  Same returns as mesh_reg; at 'uniform' / 0 the same bits."""
    if laplacian_method not in LAPLACIAN_METHODS:
        raise ValueError(f"laplacian_method must be one of {sorted(LAPLACIAN_METHODS)}, got {laplacian_method!r}")
    method = LAPLACIAN_METHODS[laplacian_method]
    t = check_edge_target_length(edge_target_length)
    if method and cot_topo is None:
        raise ValueError(f"laplacian_method {laplacian_method!r} needs the topology of mesh_losses.build_cot_topology")
    verts, target = _f32c(verts), _f32c(target)
    V = verts.shape[0]
    dev = verts.device
    E, P = topo["edges"].shape[0], topo["pairs"].shape[0]
    c = cot_topo if method else None
    F = c["faces"].shape[0] if c else 0
    if c and (tuple(c["nbr_edge"].shape) != (2 * E,) or tuple(c["edge_off"].shape) != (E + 1,) or tuple(c["edge_ref"].shape) != (3 * F,)
              or tuple(c["inc_off"].shape) != (V + 1,) or tuple(c["inc_ref"].shape) != (3 * F,)
              or tuple(topo["nbr_off"].shape) != (V + 1,) or tuple(topo["nbr_idx"].shape) != (2 * E,)):
        raise ValueError("cot_topo does not belong to this topology / vertex count")
    scratch = torch.empty((_lib.load().st3d_mesh_reg_ex_scratch_floats(V, E, F, P),), dtype=F32, device=dev)
    parts = torch.empty((4 * _lib.load().st3d_reduce_partials(),), dtype=F32, device=dev)
    out = torch.zeros((5,), dtype=F32, device=dev)
    g = torch.zeros_like(verts) if want_grad else None
    w = (ctypes.c_float * 4)(*[float(x) for x in weights])
    cp = (lambda k: dptr(c[k], I32)) if c else (lambda k: None)
    call("st3d_mesh_reg_ex", dptr(verts), dptr(target), V, dptr(topo["edges"], I32), E,
         dptr(topo["nbr_off"], I32), dptr(topo["nbr_idx"], I32), dptr(topo["pairs"], I32) if P else None, P,
         dptr(topo["pair_off"], I32) if P else None, dptr(topo["pair_ref"], I32) if P else None,
         cp("faces"), F, cp("nbr_edge"), cp("edge_off"), cp("edge_ref"), cp("inc_off"), cp("inc_ref"), method, t, w,
         dptr(scratch), dptr(parts), dptr(out), dptr(g), stream_ptr())
    return out, g


# ------------------------------------------------------------------ Chamfer loss (csrc/chamfer.hip)
CHAMFER_MAX_POINTS = 1 << 20
F64 = torch.float64


def check_num_points(n, what="num_samples"):
    """an integer in 1..2^20; else ValueError"""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= CHAMFER_MAX_POINTS:
        raise ValueError(f"{what} must be an integer in 1..{CHAMFER_MAX_POINTS}, got {n!r}")
    return n


def _cloud(t, what):
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must be (P,3), got {tuple(t.shape)}")
    check_num_points(int(t.shape[0]), f"the number of points of {what}")
    return _f32c(t)


def knn1_geometry(P1, P2):
    """-> (tile, segments) of the launch st3d_knn1 makes: segment s scans the ceil(ceil(P2 / tile) / segments) * tile points
    from s times that many on, in LDS tiles of `tile` points."""
    tile, segments = ctypes.c_int(0), ctypes.c_int(0)
    call("st3d_knn1_geometry", check_num_points(P1, "P1"), check_num_points(P2, "P2"), ctypes.byref(tile), ctypes.byref(segments))
    return tile.value, segments.value


def knn1(x, y):
    """x (P1,3), y (P2,3) -> (idx (P1) int32 = the nearest y of every x, the lowest index among equals; dist2 (P1) fp32)"""
    x, y = _cloud(x, "x"), _cloud(y, "y")
    P1, P2 = x.shape[0], y.shape[0]
    nbytes = _lib.load().st3d_knn1_workspace_bytes(P1, P2)
    ws = torch.empty((nbytes // 8,), dtype=F64, device=x.device)
    idx = torch.empty((P1,), dtype=I32, device=x.device)
    dist = torch.empty((P1,), dtype=F32, device=x.device)
    call("st3d_knn1", dptr(x), dptr(y), P1, P2, dptr(ws), nbytes, dptr(idx), dptr(dist), stream_ptr())
    return idx, dist


def face_area_cdf(verts, faces_i32):
    """-> cdf (F) fp64: the inclusive scan of the fp64 face areas.  faces_i32: range-checked (Meshes.faces_i32())."""
    verts = _f32c(verts)
    F = faces_i32.shape[0]
    nbytes = _lib.load().st3d_face_area_cdf_scratch_bytes(F)
    scratch = torch.empty((max(nbytes // 8, 1),), dtype=F64, device=verts.device)
    cdf = torch.empty((F,), dtype=F64, device=verts.device)
    call("st3d_face_area_cdf", dptr(verts), dptr(faces_i32, I32), F, dptr(scratch), nbytes, dptr(cdf), stream_ptr())
    return cdf


def sample_points_fwd(verts, faces_i32, cdf, r):
    """r (3,N) fp32 uniforms, row 0 ascending -> (points (N,3), face_idx (N) int32 ascending)"""
    verts = _f32c(verts)
    if r.dim() != 2 or r.shape[0] != 3:
        raise ValueError(f"r must be (3,N), got {tuple(r.shape)}")
    N, F = check_num_points(int(r.shape[1])), faces_i32.shape[0]
    if tuple(cdf.shape) != (F,):
        raise ValueError("cdf does not belong to these faces")
    points = torch.empty((N, 3), dtype=F32, device=verts.device)
    face_idx = torch.empty((N,), dtype=I32, device=verts.device)
    call("st3d_sample_points_fwd", dptr(verts), dptr(faces_i32, I32), F, dptr(cdf, F64), dptr(r, F32), N, dptr(points),
         dptr(face_idx), stream_ptr())
    return points, face_idx


def sample_points_bwd(grad_points, r, face_idx, F, incidence, out):
    """out (V,3) += d <grad_points, points> / d verts; incidence = render.vertex_incidence(faces_i32, V)"""
    N, V = check_num_points(int(r.shape[1])), out.shape[0]
    if tuple(grad_points.shape) != (N, 3) or tuple(face_idx.shape) != (N,):
        raise ValueError("grad_points / face_idx do not belong to r")
    if tuple(incidence[0].shape) != (V + 1,) or tuple(incidence[1].shape) != (3 * F,):
        raise ValueError("the incidence list does not belong to this mesh")
    nbytes = _lib.load().st3d_sample_points_bwd_scratch_bytes(F)
    scratch = torch.empty((nbytes // 8,), dtype=F64, device=out.device)
    call("st3d_sample_points_bwd", dptr(_f32c(grad_points)), dptr(r, F32), dptr(face_idx, I32), N, F, V, dptr(incidence[0], I32),
         dptr(incidence[1], I32), dptr(scratch), nbytes, dptr(out, F32), stream_ptr())
    return out


def chamfer_sum(dist, scale, out):
    """out (1) fp32 = (float)((double)out + scale * sum(dist)), the sum ordered, in fp64"""
    call("st3d_chamfer_sum", dptr(dist, F32), check_num_points(int(dist.numel()), "the number of distances"), float(scale),
         dptr(out, F32), stream_ptr())
    return out


def chamfer_bwd(x, y, nn, order, sorted_nn, c_self, c_other, out):
    """out (P1,3) += c_self (x_i - y[nn[i]]) + c_other sum over the y_j whose neighbour is x_i, ascending j.  nn (P1) int32 or
    None; (order, sorted_nn) (P2) int32 = torch.sort(neighbours of y in x, stable=True) indices and values, or both None."""
    x, y = _cloud(x, "x"), _cloud(y, "y")
    P1, P2 = x.shape[0], y.shape[0]
    if nn is None and order is None:
        raise ValueError("chamfer_bwd needs nn or (order, sorted_nn)")
    if (order is None) != (sorted_nn is None):
        raise ValueError("order and sorted_nn come together")
    if (nn is not None and tuple(nn.shape) != (P1,)) or (order is not None and (tuple(order.shape) != (P2,) or
                                                                                 tuple(sorted_nn.shape) != (P2,))):
        raise ValueError("index lists do not belong to these clouds")
    if tuple(out.shape) != (P1, 3):
        raise ValueError("out must be (P1,3)")
    call("st3d_chamfer_bwd", dptr(x), dptr(y), P1, P2, dptr(nn, I32), dptr(order, I32), dptr(sorted_nn, I32), float(c_self),
         float(c_other), dptr(out, F32), stream_ptr())
    return out


# ------------------------------------------------------------------ NNFM style loss (csrc/nnfm.hip)
NNFM_MAX_POSITIONS = 1 << 20
NNFM_MAX_CHANNELS = 512


def _nnfm_size(n, what, hi=NNFM_MAX_POSITIONS):
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= hi:
        raise ValueError(f"{what} must be an integer in 1..{hi}, got {n!r}")
    return n


def _nnfm_tap(t, what):
    """a tap (B,C,H,W) -> (contiguous fp32 tensor, B, C, H * W)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor (B,C,H,W)")
    if t.dim() != 4:
        raise ValueError(f"{what} must be (B,C,H,W), got {tuple(t.shape)}")
    B, C, H, W = (int(s) for s in t.shape)
    _nnfm_size(B, f"the batch of {what}", 65535)
    _nnfm_size(C, f"the channels of {what}", NNFM_MAX_CHANNELS)
    _nnfm_size(H * W, f"the positions of {what}")
    return _f32c(t), B, C, H * W


def nnfm_geometry(N, M, C):
    """-> (tile_q, tile_s, segments) of the launch st3d_nnfm_search makes: query tiles of tile_q positions; run s scans the
    ceil(ceil(M / tile_s) / segments) * tile_s style positions from s times that many on, in tiles of tile_s."""
    tq, ts, seg = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    call("st3d_nnfm_geometry", _nnfm_size(N, "N"), _nnfm_size(M, "M"), _nnfm_size(C, "C", NNFM_MAX_CHANNELS), ctypes.byref(tq),
         ctypes.byref(ts), ctypes.byref(seg))
    return tq.value, ts.value, seg.value


def nnfm_normalise(x, want_hat=True):
    """x (B,C,H,W) -> (xhat (B,C,H,W) fp32 = every position's vector over its norm, a zero vector staying zero -- or None --,
    norm (B,H*W) fp32 = sqrtf of the squares added in ascending channel order)"""
    x, B, C, M = _nnfm_tap(x, "x")
    xhat = torch.empty_like(x) if want_hat else None
    norm = torch.empty((B, M), dtype=F32, device=x.device)
    call("st3d_nnfm_normalise", dptr(x), B, C, M, dptr(xhat), dptr(norm), stream_ptr())
    return xhat, norm


def _nnfm_weights(weights, B, N):
    if weights is None:
        return None
    if not torch.is_tensor(weights):
        raise TypeError("weights must be a tensor (B,N) or (B,H,W)")
    if weights.numel() != B * N or weights.shape[0] != B:
        raise ValueError(f"weights must hold ({B},{N}) values, got {tuple(weights.shape)}")
    return _f32c(weights).reshape(B, N)


def _nnfm_style(style_hat, B, C):
    style_hat, Bs, Cs, M = _nnfm_tap(style_hat, "style_hat")
    if Cs != C:
        raise ValueError(f"style_hat has {Cs} channels, the features {C}")
    if Bs not in (1, B):
        raise ValueError(f"style_hat must hold 1 or {B} images, got {Bs}")
    return style_hat, Bs, M


def nnfm_search(feat, style_hat, weights=None, normalised=None):
    """feat (B,C,H,W) the render tap, style_hat (Bs,C,Hs,Ws) the unit-norm style tap (nnfm_normalise), Bs in {1, B}, weights
    (B,H*W) | (B,H,W) >= 0 or None -> (idx (B,N) int32 = the nearest style position of every position by cosine distance, the
    lowest index among equals, -1 where inactive or the query is zero; dist (B,N) fp32 = 1 - similarity).
    normalised = nnfm_normalise(feat) when the caller has it already."""
    feat, B, C, N = _nnfm_tap(feat, "feat")
    style_hat, Bs, M = _nnfm_style(style_hat, B, C)
    weights = _nnfm_weights(weights, B, N)
    fhat, fnorm = normalised if normalised is not None else nnfm_normalise(feat)
    nbytes = _lib.load().st3d_nnfm_workspace_bytes(B, N, M, C)
    ws = torch.empty((nbytes // 8,), dtype=F64, device=feat.device)
    idx = torch.empty((B, N), dtype=I32, device=feat.device)
    dist = torch.empty((B, N), dtype=F32, device=feat.device)
    call("st3d_nnfm_search", dptr(fhat, F32), dptr(fnorm, F32), dptr(style_hat), dptr(weights), B, Bs, C, N, M, dptr(ws), nbytes,
         dptr(idx), dptr(dist), stream_ptr())
    return idx, dist


def nnfm_sum(dist, weights=None, batch_denom=None):
    """dist (B,N), weights (B,N) or None -> (loss (1) fp32 = (1 / batch_denom) sum_b (sum_i w_i d_i / sum_i w_i), ordered,
    in fp64, rounded once; wsum (B) fp64 = sum_i w_i).  An image with sum w = 0 adds 0."""
    if dist.dim() != 2:
        raise ValueError(f"dist must be (B,N), got {tuple(dist.shape)}")
    B, N = int(dist.shape[0]), int(dist.shape[1])
    weights = _nnfm_weights(weights, B, N)
    loss = torch.empty((1,), dtype=F32, device=dist.device)
    wsum = torch.empty((B,), dtype=F64, device=dist.device)
    call("st3d_nnfm_sum", dptr(dist, F32), dptr(weights), B, N, 1.0 / float(batch_denom if batch_denom is not None else B),
         dptr(loss), dptr(wsum), stream_ptr())
    return loss, wsum


def nnfm_bwd(feat, style_hat, idx, dist, wsum, weights=None, batch_denom=None, grad_out=None):
    """-> d loss / d feat (B,C,H,W), one launch, every element written: -g (w_i / (W_b batch_denom n_i)) (s^_j - sim f^_i) with
    j = idx_i, sim = 1 - dist_i; exact zeros where idx_i = -1.  grad_out: the incoming scalar g as a device tensor, or None."""
    feat, B, C, N = _nnfm_tap(feat, "feat")
    style_hat, Bs, M = _nnfm_style(style_hat, B, C)
    weights = _nnfm_weights(weights, B, N)
    if tuple(idx.shape) != (B, N) or tuple(dist.shape) != (B, N) or tuple(wsum.shape) != (B,):
        raise ValueError("idx / dist / wsum do not belong to these features")
    if grad_out is not None:
        grad_out = _f32c(grad_out).reshape(1)
    grad = torch.empty_like(feat)
    call("st3d_nnfm_bwd", dptr(feat), dptr(style_hat), dptr(idx, I32), dptr(dist, F32), dptr(weights),
         dptr(wsum, F64), dptr(grad_out), B, Bs, C, N, M, 1.0 / float(batch_denom if batch_denom is not None else B), dptr(grad),
         stream_ptr())
    return grad


# ------------------------------------------------------------------ sliced Wasserstein style loss (csrc/swd.hip)
SWD_MAX_POSITIONS = 1 << 20
SWD_MAX_CHANNELS = 512


def _swd_size(n, what, hi=SWD_MAX_POSITIONS):
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= hi:
        raise ValueError(f"{what} must be an integer in 1..{hi}, got {n!r}")
    return n


def _swd_rows(t, what, dtype=F32):
    """(B,K,N) (or (B,K,H,W)) -> (contiguous tensor (B,K,N), B, K, N)"""
    if not torch.is_tensor(t):
        raise TypeError(f"{what} must be a tensor (B,K,N)")
    if t.dim() not in (3, 4):
        raise ValueError(f"{what} must be (B,K,N) or (B,K,H,W), got {tuple(t.shape)}")
    B, K = int(t.shape[0]), int(t.shape[1])
    N = int(t[0, 0].numel()) if B and K else 0
    _swd_size(B, f"the batch of {what}", 65535)
    _swd_size(K, f"the rows of {what}", SWD_MAX_CHANNELS)
    _swd_size(N, f"the positions of {what}")
    return t.detach().to(dtype).contiguous().reshape(B, K, N), B, K, N


def _swd_weights(weights, B, N):
    if weights is None:
        return None
    if not torch.is_tensor(weights):
        raise TypeError("weights must be a tensor (B,N) or (B,H,W)")
    if weights.numel() != B * N or weights.shape[0] != B:
        raise ValueError(f"weights must hold ({B},{N}) values, got {tuple(weights.shape)}")
    return _f32c(weights).reshape(B, N)


def _swd_style(tsorted, B, K):
    tsorted, Bs, Ks, M = _swd_rows(tsorted, "tsorted")
    if Ks != K:
        raise ValueError(f"tsorted has {Ks} rows per image, sorted {K}")
    if Bs not in (1, B):
        raise ValueError(f"tsorted must hold 1 or {B} images, got {Bs}")
    return tsorted, Bs, M


def _swd_count(count, B):
    if not torch.is_tensor(count) or tuple(count.shape) != (B,):
        raise ValueError(f"count must be a tensor ({B},)")
    return count


def swd_project(x, a):
    """x (B,Q,N) | (B,Q,H,W), a (R,Q) -> out (B,R,N) fp32, out_brn = sum_q a_rq x_bqn as ONE ascending fp32 fma chain from 0
    (the fp32 MFMA), never split over q.  1 <= Q, R <= 512."""
    x, B, Q, N = _swd_rows(x, "x")
    if not torch.is_tensor(a):
        raise TypeError("a must be a tensor (R,Q)")
    if a.dim() != 2 or int(a.shape[1]) != Q:
        raise ValueError(f"a must be (R,{Q}), got {tuple(a.shape)}")
    R = _swd_size(int(a.shape[0]), "the rows of a", SWD_MAX_CHANNELS)
    a = _f32c(a)
    out = torch.empty((B, R, N), dtype=F32, device=x.device)
    call("st3d_swd_project", dptr(x), dptr(a), B, Q, R, N, dptr(out), stream_ptr())
    return out


def swd_geometry(N):
    """-> (block, passes) of the launch st3d_swd_sort makes for rows of N positions: strides below `block` are sorted in LDS,
    `passes` launches on tiles strided in memory handle the strides from `block` up, one per level (0 when N <= block)."""
    block, passes = ctypes.c_int(0), ctypes.c_int(0)
    call("st3d_swd_geometry", _swd_size(N, "N"), ctypes.byref(block), ctypes.byref(passes))
    return block.value, passes.value


def swd_workspace_bytes(B, K, N):
    """the workspace st3d_swd_sort needs (0 when the rows fit one block)"""
    return int(_lib.load().st3d_swd_workspace_bytes(_swd_size(B, "B", 65535), _swd_size(K, "K", SWD_MAX_CHANNELS), _swd_size(N, "N")))


def swd_sort(proj, weights=None, want_perm=True):
    """proj (B,K,N), weights (B,N) | (B,H,W) >= 0 or None -> (sorted (B,K,N) fp32, perm (B,K,N) int32 or None, count (B) int32):
    every row ascending by (inactive, key, index) -- inactive = not w > 0, key = the order-preserving map of the fp32 bits with
    every NaN as 0x7FC00000 -- so the result is unique; sorted holds the original values, perm[r] the position of rank r."""
    proj, B, K, N = _swd_rows(proj, "proj")
    weights = _swd_weights(weights, B, N)
    nbytes = swd_workspace_bytes(B, K, N)
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=proj.device) if nbytes else None
    out = torch.empty_like(proj)
    perm = torch.empty((B, K, N), dtype=I32, device=proj.device) if want_perm else None
    count = torch.empty((B,), dtype=I32, device=proj.device)
    call("st3d_swd_sort", dptr(proj), dptr(weights), B, K, N, dptr(ws), nbytes, dptr(out), dptr(perm), dptr(count), stream_ptr())
    return out, perm, count


def swd_loss(sorted_rows, count, tsorted, batch_denom=None):
    """sorted_rows (B,K,N), count (B) int32, tsorted (Bs,K,M) -> loss (1) fp32 = (1 / batch_denom) sum_b (1 / (K n_b))
    sum_k sum_{r<n_b} (sorted_kbr - tsorted_{k,j(r)})^2, j(r) = ((2r+1) M) // (2 n_b); ordered, in fp64, rounded once."""
    sorted_rows, B, K, N = _swd_rows(sorted_rows, "sorted")
    tsorted, Bs, M = _swd_style(tsorted, B, K)
    count = _swd_count(count, B)
    loss = torch.empty((1,), dtype=F32, device=sorted_rows.device)
    ws = torch.empty((B * K,), dtype=F64, device=sorted_rows.device)
    call("st3d_swd_loss", dptr(sorted_rows), dptr(count, I32), dptr(tsorted), B, Bs, K, N, M,
         1.0 / float(batch_denom if batch_denom is not None else B), dptr(ws), B * K * 8, dptr(loss), stream_ptr())
    return loss


def swd_bwd(sorted_rows, perm, count, tsorted, batch_denom=None, grad_out=None):
    """-> d loss / d proj (B,K,N), one launch, every element written once through perm: g 2 / (batch_denom K n_b)
    (sorted_kbr - tsorted_{k,j(r)}) at position perm[r] for r < n_b, an exact +0 elsewhere.  grad_out: the incoming scalar g
    as a device tensor, or None."""
    sorted_rows, B, K, N = _swd_rows(sorted_rows, "sorted")
    tsorted, Bs, M = _swd_style(tsorted, B, K)
    count = _swd_count(count, B)
    if not torch.is_tensor(perm) or tuple(perm.shape) != (B, K, N):
        raise ValueError("perm does not belong to these rows")
    if grad_out is not None:
        grad_out = _f32c(grad_out).reshape(1)
    gproj = torch.empty_like(sorted_rows)
    call("st3d_swd_bwd", dptr(sorted_rows), dptr(perm, I32), dptr(count, I32), dptr(tsorted), dptr(grad_out), B, Bs, K, N, M,
         1.0 / float(batch_denom if batch_denom is not None else B), dptr(gproj), stream_ptr())
    return gproj


# ------------------------------------------------------------------ general soft renderer (K faces per pixel, blur)
def raster_soft_fwd(verts_ndc, faces_i32, S, K, blur_radius=0.0, clip_bary=None, cull_backfaces=False,
                    perspective_correct=True, z_clip=None):
    """-> pix_to_face (B,S,S,K) int32, zbuf, bary (B,S,S,K,3), dists; clip_bary None = PyTorch3D default (blur > 0).
    z_clip: near-plane clipping depth (PyTorch3D: znear / 2); then a fifth tensor, the record slot of every fragment,
    is returned for raster_soft_bwd."""
    B, V, _ = verts_ndc.shape
    F = faces_i32.shape[0]
    dev = verts_ndc.device
    if clip_bary is None:
        clip_bary = blur_radius > 0.0
    slots = None
    if z_clip is None:
        ws_bytes = _lib.load().st3d_raster_workspace_bytes(B, F)
        rec = torch.empty((ws_bytes // 4,), dtype=F32, device=dev)
        call("st3d_face_setup", dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, F, dptr(rec), ws_bytes, stream_ptr())
    else:
        ws_bytes = _lib.load().st3d_clip_records_bytes(B, F)
        rec = torch.empty((ws_bytes // 4,), dtype=F32, device=dev)
        call("st3d_face_setup_clip", dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, F, float(z_clip),
             1 if perspective_correct else 0, dptr(rec), ws_bytes, stream_ptr())
        slots = torch.empty((B, S, S, K), dtype=I32, device=dev)
    p2f = torch.empty((B, S, S, K), dtype=I32, device=dev)
    zbuf = torch.empty((B, S, S, K), dtype=F32, device=dev)
    bary = torch.empty((B, S, S, K, 3), dtype=F32, device=dev)
    dists = torch.empty((B, S, S, K), dtype=F32, device=dev)
    call("st3d_raster_soft_fwd", dptr(rec), B, F, S, int(K), float(blur_radius), 1 if clip_bary else 0,
         1 if cull_backfaces else 0, 1 if perspective_correct else 0, 1 if slots is None else 2, dptr(slots), dptr(p2f),
         dptr(zbuf), dptr(bary), dptr(dists), stream_ptr())
    return (p2f, zbuf, bary, dists) if slots is None else (p2f, zbuf, bary, dists, slots)


def _bg3(background):
    return (ctypes.c_float * 3)(*[float(x) for x in background])


def shade_soft_fwd(frag, verts_uvs, faces_uvs_i32, texture, sigma=1e-4, gamma=1e-4, background=(1.0, 1.0, 1.0)):
    B, S, _, K = frag[0].shape
    rgb, alpha = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_soft_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, texture.shape[0], K,
         float(sigma), float(gamma), _bg3(background), dptr(rgb), dptr(alpha), stream_ptr())
    return rgb, alpha


def _soft_grads(T, B, S, K, want_texture, want_geometry, dev):
    """-> grad_texture (T,T,3) zeros | None, (grad_bary (B,S,S,K,3), grad_zbuf (B,S,S,K), grad_dists (B,S,S,K)) | None"""
    gt = torch.zeros((T, T, 3), dtype=F32, device=dev) if want_texture else None
    if not want_geometry:
        return gt, None
    return gt, (torch.empty((B, S, S, K, 3), dtype=F32, device=dev), torch.empty((B, S, S, K), dtype=F32, device=dev),
                torch.empty((B, S, S, K), dtype=F32, device=dev))


def shade_soft_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, sigma=1e-4, gamma=1e-4, background=(1.0, 1.0, 1.0),
                   want_texture=True, want_geometry=True):
    """-> (grad_texture (T,T,3) | None, (grad_bary, grad_zbuf, grad_dists) | None)"""
    B, S, _, K = frag[0].shape
    T = texture.shape[0]
    gt, geo = _soft_grads(T, B, S, K, want_texture, want_geometry, frag[0].device)
    gb, gz, gd = geo or (None, None, None)
    head = (dptr(grad_rgb.contiguous(), F32), *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, T, K,
            float(sigma), float(gamma), _bg3(background), dptr(gt), dptr(gb), dptr(gz), dptr(gd))
    if _DETERMINISTIC and gt is not None:       # fixed-point texture scatter: bitwise reproducible
        ws, nb = _det_ws(_lib.load().st3d_shade_soft_bwd_det_workspace_bytes(T), frag[0].device)
        call("st3d_shade_soft_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_shade_soft_bwd", *head, stream_ptr())
    return gt, geo


def raster_soft_bwd(grads, p2f, verts_ndc, faces_i32, clip_bary, perspective_correct=True, slots=None, z_clip=None):
    gb, gz, gd = grads
    B, V, _ = verts_ndc.shape
    S, K = p2f.shape[1], p2f.shape[3]
    g = torch.empty((B, V, 3), dtype=F32, device=verts_ndc.device)
    head = (dptr(gb, F32), dptr(gz, F32), dptr(gd, F32), dptr(p2f, I32), dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V,
            faces_i32.shape[0], S, K, 1 if clip_bary else 0, 1 if perspective_correct else 0, dptr(slots, I32),
            float(z_clip) if z_clip is not None else 0.0, dptr(g))
    if _DETERMINISTIC:                          # fixed-point vertex scatter
        ws, nb = _det_ws(_lib.load().st3d_raster_soft_bwd_det_workspace_bytes(B, V, S), verts_ndc.device)
        call("st3d_raster_soft_bwd_det", *head, dptr(ws), nb, stream_ptr())
    else:
        call("st3d_raster_soft_bwd", *head, stream_ptr())
    return g


# ------------------------------------------------------------------ silhouette (csrc/silhouette.hip)
def _check_sigma(sigma):
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be positive")
    return float(sigma)


def silhouette_fwd(p2f, dists, sigma=1e-4):
    """sigmoid_alpha_blend's alpha of the fragments (p2f, dists) (B,S,S,K) -> (B,1,S,S); no texture, UVs or barycentrics."""
    sigma = _check_sigma(sigma)
    B, S, _, K = p2f.shape
    alpha = torch.empty((B, 1, S, S), dtype=F32, device=p2f.device)
    call("st3d_silhouette_fwd", dptr(p2f, I32), dptr(dists, F32), B, S, K, sigma, dptr(alpha), stream_ptr())
    return alpha


def silhouette_bwd(grad_alpha, p2f, dists, sigma=1e-4, out=None):
    """grad_alpha (B,1,S,S) -> grad_dists (B,S,S,K); `out`: an existing grad_dists the result is ADDED to."""
    sigma = _check_sigma(sigma)
    B, S, _, K = p2f.shape
    acc = 1
    if out is None:
        out = torch.empty((B, S, S, K), dtype=F32, device=p2f.device)
        acc = 0
    call("st3d_silhouette_bwd", dptr(grad_alpha.contiguous(), F32), dptr(p2f, I32), dptr(dists, F32), B, S, K, sigma, acc,
         dptr(out, F32), stream_ptr())
    return out


def silhouette_loss(p2f, dists, target, sigma=1e-4, scale=1.0, want_grad=True):
    """-> (loss (1,) = scale * sum (alpha - target)^2, grad_dists (B,S,S,K) | None) in one pass; target (B,1,S,S)."""
    sigma = _check_sigma(sigma)
    B, S, _, K = p2f.shape
    if target.numel() != B * S * S:
        raise ValueError(f"target must hold {B}x1x{S}x{S} values, got {tuple(target.shape)}")
    dev = p2f.device
    parts = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=dev)
    out = torch.zeros((1,), dtype=F32, device=dev)
    gd = torch.empty((B, S, S, K), dtype=F32, device=dev) if want_grad else None
    call("st3d_silhouette_loss", dptr(p2f, I32), dptr(dists, F32), dptr(target.contiguous(), F32), B, S, K, sigma, float(scale),
         dptr(gd), dptr(parts), dptr(out), stream_ptr())
    return out, gd


# ------------------------------------------------------------------ silhouette rasteriser (csrc/silraster.hip)
SILRASTER_MAX_FACES_PER_PIXEL = 64


def _check_silraster_k(K):
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= SILRASTER_MAX_FACES_PER_PIXEL:
        raise ValueError(f"faces_per_pixel must be an integer in 1..{SILRASTER_MAX_FACES_PER_PIXEL}, got {K!r}")
    return int(K)


def _silraster_records(verts_ndc, faces_i32, perspective_correct, z_clip):
    """the two clipped records per face of st3d_face_setup_clip (B*F*96 bytes; recomputed in the backward, never kept)"""
    B, V, _ = verts_ndc.shape
    F = faces_i32.shape[0]
    nb = _lib.load().st3d_clip_records_bytes(B, F)
    rec = torch.empty((nb // 4,), dtype=F32, device=verts_ndc.device)
    call("st3d_face_setup_clip", dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, F, float(z_clip),
         1 if perspective_correct else 0, dptr(rec), nb, stream_ptr())
    return rec


def _silraster_common(S, blur_radius, clip_bary, cull_backfaces, perspective_correct):
    return (int(S), float(blur_radius), 1 if clip_bary else 0, 1 if cull_backfaces else 0, 1 if perspective_correct else 0)


def silraster_fwd(verts_ndc, faces_i32, S, K, blur_radius, sigma=1e-4, clip_bary=True, cull_backfaces=False,
                  perspective_correct=True, z_clip=0.5):
    """SoftSilhouetteShader's alpha at faces_per_pixel K = 1..64 without fragments: -> (alpha (B,1,S,S), state (3,B,S,S));
    state (12 bytes per pixel whatever K is) is what silraster_bwd needs."""
    K, sigma = _check_silraster_k(K), _check_sigma(sigma)
    B, F, dev = verts_ndc.shape[0], faces_i32.shape[0], verts_ndc.device
    rec = _silraster_records(verts_ndc, faces_i32, perspective_correct, z_clip)
    S, blur, clip, cull, persp = _silraster_common(S, blur_radius, clip_bary, cull_backfaces, perspective_correct)
    alpha = torch.empty((B, 1, S, S), dtype=F32, device=dev)
    state = torch.empty((3, B, S, S), dtype=F32, device=dev)
    call("st3d_silraster_fwd", dptr(rec), B, F, S, K, blur, clip, cull, persp, sigma, dptr(alpha), dptr(state), stream_ptr())
    return alpha, state


def silraster_loss(verts_ndc, faces_i32, target, K, blur_radius, sigma=1e-4, scale=1.0, clip_bary=True, cull_backfaces=False,
                   perspective_correct=True, z_clip=0.5):
    """-> (loss (1,) = scale * sum (alpha - target)^2, state (4,B,S,S)) in one raster pass; target (B,1,S,S).  alpha does
    not reach memory; plane 3 of state is alpha - target, which silraster_bwd(grad_scale = 2 * scale) turns into d/d verts."""
    K, sigma = _check_silraster_k(K), _check_sigma(sigma)
    B, F, dev = verts_ndc.shape[0], faces_i32.shape[0], verts_ndc.device
    if target.dim() != 4 or target.shape[0] != B or target.shape[2] != target.shape[3] or target.numel() != B * target.shape[2] ** 2:
        raise ValueError(f"target must be ({B},1,S,S), got {tuple(target.shape)}")
    rec = _silraster_records(verts_ndc, faces_i32, perspective_correct, z_clip)
    S, blur, clip, cull, persp = _silraster_common(target.shape[2], blur_radius, clip_bary, cull_backfaces, perspective_correct)
    state = torch.empty((4, B, S, S), dtype=F32, device=dev)
    parts = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=dev)
    out = torch.zeros((1,), dtype=F32, device=dev)
    call("st3d_silraster_loss", dptr(rec), B, F, S, K, blur, clip, cull, persp, sigma, dptr(target.contiguous(), F32),
         float(scale), dptr(state), dptr(parts), dptr(out), stream_ptr())
    return out, state


def silraster_bwd(state, verts_ndc, faces_i32, blur_radius, sigma=1e-4, grad_alpha=None, grad_scale=1.0, clip_bary=True,
                  cull_backfaces=False, perspective_correct=True, z_clip=0.5):
    """d/d verts_ndc (B,V,3) of silraster_fwd (grad_alpha (B,1,S,S)) or of silraster_loss (grad_alpha None, grad_scale =
    2 * scale) from the saved state; the raster settings must be the forward's."""
    sigma = _check_sigma(sigma)
    B, V, _ = verts_ndc.shape
    F, dev = faces_i32.shape[0], verts_ndc.device
    if state.dim() != 4 or state.shape[0] != (3 if grad_alpha is not None else 4) or state.shape[1] != B:
        raise ValueError(f"state {tuple(state.shape)} does not belong to this call")
    rec = _silraster_records(verts_ndc, faces_i32, perspective_correct, z_clip)
    S, blur, clip, cull, persp = _silraster_common(state.shape[2], blur_radius, clip_bary, cull_backfaces, perspective_correct)
    g = torch.empty((B, V, 3), dtype=F32, device=dev)
    ws, nb = _det_ws(_lib.load().st3d_silraster_bwd_workspace_bytes(B, V, S), dev) if _DETERMINISTIC else (None, 0)
    ga = grad_alpha.to(F32).contiguous() if grad_alpha is not None else None
    call("st3d_silraster_bwd", dptr(rec), dptr(verts_ndc, F32), dptr(faces_i32, I32), B, V, F, S, blur, clip, cull, persp,
         float(z_clip), sigma, dptr(state, F32), dptr(ga, F32), float(grad_scale), dptr(g), dptr(ws), nb, stream_ptr())
    return g


# ------------------------------------------------------------------ Phong lighting (csrc/phong.h, csrc/lighting.hip)
# `lit` below is st3d.render.LitSetup: verts (V,3), normals (V,3) or None, faces_i32, R (B,3,3), T (B,3), block (n,24),
# kind, weight_bound (see include/st3d.h)
def vertex_normals(verts, faces_i32, incidence):
    """-> (normals (V,3), unnormalised sums (V,3)); incidence = (inc_off (V+1), inc_ref (3F)) int32."""
    verts = _f32c(verts)
    V, F = verts.shape[0], faces_i32.shape[0]
    dev = verts.device
    scratch = torch.empty((_lib.load().st3d_vertex_normals_scratch_floats(F),), dtype=F32, device=dev)
    n = torch.empty((V, 3), dtype=F32, device=dev)
    m = torch.empty((V, 3), dtype=F32, device=dev)
    call("st3d_vertex_normals", dptr(verts), dptr(faces_i32, I32), V, F, dptr(incidence[0], I32), dptr(incidence[1], I32),
         dptr(scratch), dptr(n), dptr(m), stream_ptr())
    return n, m


def vertex_normals_bwd(verts, faces_i32, incidence, unnormalised, grad_normals, grad_pos, out):
    """out (V,3) += grad_pos (or nothing) + d/dverts <grad_normals, normals(verts)>."""
    verts = _f32c(verts)
    V, F = verts.shape[0], faces_i32.shape[0]
    scratch = torch.empty((_lib.load().st3d_vertex_normals_scratch_floats(F),), dtype=F32, device=verts.device)
    call("st3d_vertex_normals_bwd", dptr(verts), dptr(faces_i32, I32), V, F, dptr(incidence[0], I32), dptr(incidence[1], I32),
         dptr(unnormalised, F32), dptr(grad_normals.contiguous(), F32), dptr(grad_pos.contiguous(), F32) if grad_pos is not None
         else None, dptr(scratch), dptr(out, F32), stream_ptr())
    return out


def _lit_ptrs(lit):
    return (dptr(lit.verts, F32) if lit.normals is not None else None, dptr(lit.normals, F32) if lit.normals is not None else None,
            dptr(lit.faces_i32, I32), dptr(lit.R, F32), dptr(lit.T, F32), dptr(lit.block, F32), lit.block.shape[0], lit.kind)


def _lit_grads(T, B, s, want_texture, want_geometry, dev):
    """-> grad_texture (T,T,3) zeros | None, grad_bary (B,s,s,3) | None, grad_np (B,s,s,6) | None, det workspace | None, its
    bytes"""
    gt = torch.zeros((T, T, 3), dtype=F32, device=dev) if want_texture else None
    gb = torch.empty((B, s, s, 3), dtype=F32, device=dev) if want_geometry else None
    gnp = torch.empty((B, s, s, 6), dtype=F32, device=dev) if want_geometry else None
    if _DETERMINISTIC and gt is not None:
        return (gt, gb, gnp) + _det_ws(_lib.load().st3d_shade_bwd_det_workspace_bytes(T), dev)
    return gt, gb, gnp, None, 0


def shade_lit_fwd(frag, verts_uvs, faces_uvs_i32, texture, lit):
    B, S, _ = frag[0].shape
    rgb, mask = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_lit_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, texture.shape[0],
         faces_uvs_i32.shape[0], verts_uvs.shape[0], *_lit_ptrs(lit), dptr(rgb), dptr(mask), stream_ptr())
    return rgb, mask


def shade_lit_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, lit, want_texture=True, want_geometry=False):
    """-> (grad_texture (T,T,3) | None, grad_bary (B,S,S,3) | None, grad_np (B,S,S,6) | None)"""
    B, S, _ = frag[0].shape
    T = texture.shape[0]
    gt, gb, gnp, ws, nb = _lit_grads(T, B, S, want_texture, want_geometry, frag[0].device)
    call("st3d_shade_lit_bwd", dptr(grad_rgb.contiguous(), F32), *_frag_head(frag),
         *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, T, faces_uvs_i32.shape[0], verts_uvs.shape[0], *_lit_ptrs(lit),
         float(lit.weight_bound), dptr(gt), dptr(gb), dptr(gnp), dptr(ws), nb, stream_ptr())
    return gt, gb, gnp


def shade_ss_lit_fwd(frag, verts_uvs, faces_uvs_i32, texture, lit, a):
    B, S = _ss_side(frag[0], a)
    rgb, cov = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_ss_lit_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, a, texture.shape[0],
         faces_uvs_i32.shape[0], verts_uvs.shape[0], *_lit_ptrs(lit), dptr(rgb), dptr(cov), stream_ptr())
    return rgb, cov


def shade_ss_lit_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, lit, a, want_texture=True, want_geometry=False):
    """-> (grad_texture (T,T,3) | None, grad_bary (B,aS,aS,3) | None, grad_np (B,aS,aS,6) | None)"""
    B, S = _ss_side(frag[0], a)
    T = texture.shape[0]
    if tuple(grad_rgb.shape) != (B, 3, S, S):
        raise ValueError(f"grad_rgb must be {(B, 3, S, S)}, got {tuple(grad_rgb.shape)}")
    gt, gb, gnp, ws, nb = _lit_grads(T, B, a * S, want_texture, want_geometry, frag[0].device)
    call("st3d_shade_ss_lit_bwd", dptr(grad_rgb.contiguous(), F32), *_frag_head(frag),
         *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, a, T, faces_uvs_i32.shape[0], verts_uvs.shape[0], *_lit_ptrs(lit),
         float(lit.weight_bound), dptr(gt), dptr(gb), dptr(gnp), dptr(ws), nb, stream_ptr())
    return gt, gb, gnp


def shade_soft_lit_fwd(frag, verts_uvs, faces_uvs_i32, texture, lit, sigma=1e-4, gamma=1e-4, background=(1.0, 1.0, 1.0)):
    B, S, _, K = frag[0].shape
    rgb, alpha = _rgb_mask(B, S, frag[0].device)
    call("st3d_shade_soft_lit_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, texture.shape[0],
         K, float(sigma), float(gamma), _bg3(background), *_lit_ptrs(lit), dptr(rgb), dptr(alpha), stream_ptr())
    return rgb, alpha


def shade_soft_lit_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, texture, lit, sigma=1e-4, gamma=1e-4,
                       background=(1.0, 1.0, 1.0), want_texture=True, want_geometry=True):
    """-> (grad_texture | None, (grad_bary, grad_zbuf, grad_dists) | None, grad_np (B,S,S,K,6) | None)"""
    B, S, _, K = frag[0].shape
    T, dev = texture.shape[0], frag[0].device
    gt, geo = _soft_grads(T, B, S, K, want_texture, want_geometry, dev)
    gb, gz, gd = geo or (None, None, None)
    gnp = torch.empty((B, S, S, K, 6), dtype=F32, device=dev) if want_geometry else None
    ws, nb = (_det_ws(_lib.load().st3d_shade_soft_bwd_det_workspace_bytes(T), dev) if _DETERMINISTIC and gt is not None
              else (None, 0))
    call("st3d_shade_soft_lit_bwd", dptr(grad_rgb.contiguous(), F32), *_frag_head(frag),
         *_uv_head(verts_uvs, faces_uvs_i32, texture), B, S, T, K, float(sigma), float(gamma), _bg3(background),
         *_lit_ptrs(lit), float(lit.weight_bound), dptr(gt), dptr(gb), dptr(gz), dptr(gd), dptr(gnp), dptr(ws), nb,
         stream_ptr())
    return gt, geo, gnp


def phong_scatter(grad_np, p2f, bary, faces_i32, V):
    """grad_np (B,S,S[,K],6) -> (2,V,3): d/d(vertex positions), d/d(vertex normals), summed over the views."""
    B, S = p2f.shape[0], p2f.shape[1]
    K = p2f.shape[3] if p2f.dim() == 4 else 1
    dev = p2f.device
    out = torch.empty((2, V, 3), dtype=F32, device=dev)
    ws, nb = _det_ws(_lib.load().st3d_phong_scatter_workspace_bytes(B, V, S), dev) if _DETERMINISTIC else (None, 0)
    call("st3d_phong_scatter", dptr(grad_np, F32), dptr(p2f, I32), dptr(bary, F32), dptr(faces_i32, I32), B, V,
         faces_i32.shape[0], S, K, dptr(out), dptr(ws), nb, stream_ptr())
    return out


def apply_background(img, mask, bg=None):
    B, _, S, _ = img.shape
    out = torch.empty_like(img)
    bgb = 1 if (bg is None or bg.dim() == 3 or bg.shape[0] == 1) else B
    call("st3d_apply_background", dptr(img.contiguous(), F32), dptr(mask.contiguous(), F32),
         dptr(bg.contiguous(), F32) if bg is not None else None, bgb, B, S, dptr(out), stream_ptr())
    return out


# ------------------------------------------------------------------ conv / pool
def conv3x3_pack(w):
    """w (Cout,Cin,3,3) -> (w_fwd_packed, w_dgrad_packed) flat float tensors."""
    w = _f32c(w)
    Cout, Cin = w.shape[:2]
    n = _lib.load().st3d_conv3x3_packed_floats(Cout, Cin)
    wf = torch.empty((n,), dtype=F32, device=w.device)
    wd = torch.empty((n,), dtype=F32, device=w.device)
    call("st3d_conv3x3_pack", dptr(w), Cout, Cin, dptr(wf), dptr(wd), stream_ptr())
    return wf, wd


def conv3x3_fwd(x, wf, bias, Cout, relu=True):
    N, Cin, H, W = x.shape
    y = torch.empty((N, Cout, H, W), dtype=F32, device=x.device)
    call("st3d_conv3x3_fwd", dptr(x.contiguous(), F32), dptr(wf, F32), dptr(bias, F32) if bias is not None else None,
         dptr(y), N, Cin, Cout, H, W, 1 if relu else 0, stream_ptr())
    return y


def conv3x3_dgrad(gy, act, wd, Cin):
    N, Cout, H, W = gy.shape
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy.device)
    call("st3d_conv3x3_dgrad", dptr(gy.contiguous(), F32), dptr(act, F32) if act is not None else None, dptr(wd, F32),
         dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def conv1_bwd(gy, act, D, coef, wd):
    """gx (N,3,H,W) = conv1_1^T(gate(gy + coef * D act)) in one pass (st3d_conv1_bwd); gy or D may be None."""
    N, C, H, W = act.shape
    nb = _lib.load().st3d_conv1_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((nb // 4,), dtype=F32, device=act.device)
    gx = torch.empty((N, 3, H, W), dtype=F32, device=act.device)
    call("st3d_conv1_bwd", dptr(gy, F32), dptr(act, F32), dptr(D, F32), float(coef), dptr(wd, F32), dptr(ws), nb, dptr(gx),
         N, H, W, stream_ptr())
    return gx


def conv1_bwd_masked(gy, act, D, coef, wd, seg, mask):
    """conv1_bwd at the pixels of mask (N,H,W uint8), exactly 0 elsewhere; seg (N,H,W/64 uint8) from need_build."""
    N, C, H, W = act.shape
    nb = _lib.load().st3d_conv1_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((nb // 4,), dtype=F32, device=act.device)
    gx = torch.empty((N, 3, H, W), dtype=F32, device=act.device)
    call("st3d_conv1_bwd_masked", dptr(gy, F32), dptr(act, F32), dptr(D, F32), float(coef), dptr(wd, F32), dptr(ws), nb,
         dptr(gx), N, H, W, dptr(seg, U8), dptr(mask, U8), stream_ptr())
    return gx


def conv1_bwd_weighted(gy, act, D, coef, wd, w0, seg=None, mask=None):
    """gx = conv1_1^T(gate(gy + coef * D (w0 act))), w0 (N,H,W) one weight per pixel (st3d_conv1_bwd_weighted); with seg and
    mask: at the pixels of mask only, as conv1_bwd_masked."""
    N, C, H, W = act.shape
    nb = _lib.load().st3d_conv1_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((nb // 4,), dtype=F32, device=act.device)
    gx = torch.empty((N, 3, H, W), dtype=F32, device=act.device)
    if w0.numel() != N * H * W:
        raise _lib.St3dError(f"w0 has {w0.numel()} values for {N} x {H} x {W} pixels")
    call("st3d_conv1_bwd_weighted", dptr(gy, F32), dptr(act, F32), dptr(D, F32), float(coef), dptr(wd, F32), dptr(ws), nb,
         dptr(gx), N, H, W, dptr(w0.contiguous(), F32), dptr(seg, U8), dptr(mask, U8), stream_ptr())
    return gx


def need_levels(S):
    return _lib.load().st3d_need_levels(int(S))


def wino43_tile_geometry(H, W):
    """(rows, cols) of the F(4x4,3x3) kernel's output tiles on an H x W map; None where it does not cover the map."""
    r, c = ctypes.c_int(), ctypes.c_int()
    ok = _lib.load().st3d_wino43_tile_geometry(int(H), int(W), ctypes.byref(r), ctypes.byref(c))
    return (r.value, c.value) if ok else None


def need_build(mask, levels=None):
    """mask (N,S,S) uint8 -> (seg (N,S,S/64) uint8, [(list, count)] per tile level): st3d_need_build.  The lists are sized
    for every tile; only the first `count` entries (a device int32 scalar) are meaningful."""
    N, S, _ = mask.shape
    levels = need_levels(S) if levels is None else levels
    seg = torch.empty((N, S, S // 64), dtype=U8, device=mask.device)
    counts = torch.zeros((2,), dtype=I32, device=mask.device)
    lists = []
    for l in range(levels - 1):
        rows, cols = wino43_tile_geometry(S >> l, S >> l)
        lists.append(torch.full((N * ((S >> l) // rows) * ((S >> l) // cols),), -1, dtype=I32, device=mask.device))
    nb = _lib.load().st3d_need_workspace_bytes(N, S)
    ws = torch.empty((max(nb, 1),), dtype=U8, device=mask.device)
    call("st3d_need_build", dptr(mask, U8), N, S, levels, dptr(seg), dptr(ws), nb, dptr(lists[0]) if lists else None,
         dptr(lists[1]) if len(lists) > 1 else None, dptr(counts), stream_ptr())
    return seg, [(lst, counts[i]) for i, lst in enumerate(lists)]


def need_blocks_lists(S):
    return _lib.load().st3d_need_blocks_lists(int(S))


def need_blocks_build(mask, nlists=None, tile_cols=None, gram=False):
    """mask (N,S,S) uint8 -> (seg (N,S,S/64) uint8, [(list, count)] per list): the per-block need lists of the input
    gradients of conv1_2, conv2_1, conv2_2, conv3_1, conv3_2, conv3_3 (st3d_need_blocks_build).  tile_cols: 64 / 32 / 16 / 0
    per list (0 or None = the kernel's own geometry for the map; 16 = strips of 4 x 16 pixels, four entries to a step, every
    image padded with -1 to whole steps, the count in steps).  Lists are sized for every tile (strip) and start as -1.
    gram=True: a third value, (list, count) of the 64-pixel runs of the relu2_1 Gram backward (gram_bwd_gated_segs)."""
    lib = _lib.load()
    N, S, _ = mask.shape
    nlists = need_blocks_lists(S) if nlists is None else nlists
    seg = torch.empty((N, S, S // 64), dtype=U8, device=mask.device)
    counts = torch.zeros((max(nlists, 1),), dtype=I32, device=mask.device)
    tcols = [int(c or 0) for c in (tile_cols or [0] * nlists)]
    lists = [torch.full((lib.st3d_need_blocks_entries(N, S, k, tcols[k]),), -1, dtype=I32, device=mask.device) for k in range(nlists)]
    nb = lib.st3d_need_blocks_workspace_bytes(N, S)
    ws = torch.empty((max(nb, 1),), dtype=U8, device=mask.device)
    cols = (ctypes.c_int * max(nlists, 1))(*tcols)
    ptrs = (ctypes.c_void_p * max(nlists, 1))(*[l.data_ptr() for l in lists])
    glist = torch.full((lib.st3d_need_blocks_gram_runs(N, S),), -1, dtype=I32, device=mask.device) if gram else None
    gcount = torch.zeros((1,), dtype=I32, device=mask.device) if gram else None
    call("st3d_need_blocks_build", dptr(mask, U8), N, S, nlists, cols, dptr(seg), dptr(ws), nb, ptrs, dptr(counts), dptr(glist),
         dptr(gcount), stream_ptr())
    out = [(lst, counts[i]) for i, lst in enumerate(lists)]
    return (seg, out, (glist, gcount[0])) if gram else (seg, out)


def gram_bwd_gated_segs(D, feat, coef, seg_list, seg_count, out, accumulate=False, q=None):
    """The gated Gram backward over the first seg_count (device int32 scalar) entries of seg_list (device int32: image * (HW /
    64) + 64-pixel run), written into `out` (B,128,H,W) in place; the other runs are left alone (st3d_gram_bwd_gated_segs)."""
    B, C = feat.shape[:2]
    HW = feat.shape[2] * feat.shape[3]
    assert out.shape == feat.shape
    call("st3d_gram_bwd_gated_segs", dptr(D, F32), dptr(feat, F32), dptr(q, F32), B, C, HW, float(coef), 1 if accumulate else 0,
         dptr(seg_list, I32), dptr(seg_count, I32), dptr(out, F32), stream_ptr())
    return out


def conv3x3_dgrad_unpool(gy_pooled, pool_idx, pooled, wd, Cin):
    N, Cout, Hp, Wp = gy_pooled.shape
    H, W = 2 * Hp, 2 * Wp
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy_pooled.device)
    call("st3d_conv3x3_dgrad_unpool", dptr(gy_pooled.contiguous(), F32), dptr(pool_idx, U8), dptr(pooled, F32),
         dptr(wd, F32), dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def wino_pack(w):
    """w (Cout,Cin,3,3) -> (u_fwd [16][Cin][Cout], u_dgrad [16][Cout][Cin]) flat tensors."""
    w = _f32c(w)
    Cout, Cin = w.shape[:2]
    n = _lib.load().st3d_wino_packed_floats(Cout, Cin)
    uf = torch.empty((n,), dtype=F32, device=w.device)
    ud = torch.empty((n,), dtype=F32, device=w.device)
    call("st3d_wino_pack", dptr(w), Cout, Cin, dptr(uf), dptr(ud), stream_ptr())
    return uf, ud


def wino_fwd(x, uf, bias, Cout, relu=True, pool=False, keep_full=True):
    N, Cin, H, W = x.shape
    y = torch.empty((N, Cout, H, W), dtype=F32, device=x.device) if (keep_full or not pool) else None
    yp = torch.empty((N, Cout, H // 2, W // 2), dtype=F32, device=x.device) if pool else None
    idx = torch.empty((N, Cout, H // 2, W // 2), dtype=U8, device=x.device) if pool else None
    call("st3d_wino_fwd", dptr(x.contiguous(), F32), dptr(uf, F32), dptr(bias, F32) if bias is not None else None, dptr(y),
         dptr(yp), dptr(idx), N, Cin, Cout, H, W, 1 if relu else 0, stream_ptr())
    return (y, yp, idx) if pool else y


def wino_dgrad(gy, act, ud, Cin):
    N, Cout, H, W = gy.shape
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy.device)
    call("st3d_wino_dgrad", dptr(gy.contiguous(), F32), dptr(act, F32) if act is not None else None, dptr(ud, F32),
         dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def wino_dgrad_unpool(gy_pooled, pool_idx, pooled, ud, Cin):
    N, Cout, Hp, Wp = gy_pooled.shape
    H, W = 2 * Hp, 2 * Wp
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy_pooled.device)
    call("st3d_wino_dgrad_unpool", dptr(gy_pooled.contiguous(), F32), dptr(pool_idx, U8), dptr(pooled, F32), dptr(ud, F32),
         dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def wino_dgrad_chain(gy, ud, Cin, act=None, pool_idx=None, pooled=None, out_gate=None, add_target=None, add_coef=0.0):
    """One link of the producer-gated backward chain (st3d_wino_dgrad_chain)."""
    N, Cout = gy.shape[:2]
    H, W = (2 * gy.shape[2], 2 * gy.shape[3]) if pool_idx is not None else gy.shape[2:]
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy.device)
    call("st3d_wino_dgrad_chain", dptr(gy.contiguous(), F32), dptr(act, F32), dptr(pool_idx, U8), dptr(pooled, F32),
         dptr(ud, F32), dptr(out_gate, F32), dptr(add_target, F32), float(add_coef), dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def wino43_pack(w):
    """w (Cout,Cin,3,3) -> (u_fwd, u_dgrad): F(4x4,3x3) filter packs (36 floats per weight, st3d_wino43_pack)."""
    w = _f32c(w)
    Cout, Cin = w.shape[:2]
    n = _lib.load().st3d_wino43_packed_floats(Cout, Cin)
    uf = torch.empty((n,), dtype=F32, device=w.device)
    ud = torch.empty((n,), dtype=F32, device=w.device)
    call("st3d_wino43_pack", dptr(w), Cout, Cin, dptr(uf), dptr(ud), stream_ptr())
    return uf, ud


def wino43_fwd(x, uf, bias, Cout, relu=True, pool=False, keep_full=True):
    N, Cin, H, W = x.shape
    y = torch.empty((N, Cout, H, W), dtype=F32, device=x.device) if (keep_full or not pool) else None
    yp = torch.empty((N, Cout, H // 2, W // 2), dtype=F32, device=x.device) if pool else None
    idx = torch.empty((N, Cout, H // 2, W // 2), dtype=U8, device=x.device) if pool else None
    call("st3d_wino43_fwd", dptr(x.contiguous(), F32), dptr(uf, F32), dptr(bias, F32) if bias is not None else None, dptr(y),
         dptr(yp), dptr(idx), N, Cin, Cout, H, W, 1 if relu else 0, stream_ptr())
    return (y, yp, idx) if pool else y


def wino43_dgrad_chain(gy, ud, Cin, pool_idx=None, out_gate=None, add_target=None, add_coef=0.0):
    """One link of the producer-gated backward chain on the F(4x4,3x3) kernel (st3d_wino43_dgrad_chain)."""
    N, Cout = gy.shape[:2]
    H, W = (2 * gy.shape[2], 2 * gy.shape[3]) if pool_idx is not None else gy.shape[2:]
    gx = torch.empty((N, Cin, H, W), dtype=F32, device=gy.device)
    call("st3d_wino43_dgrad_chain", dptr(gy.contiguous(), F32), dptr(pool_idx, U8), dptr(ud, F32), dptr(out_gate, F32),
         dptr(add_target, F32), float(add_coef), dptr(gx), N, Cin, Cout, H, W, stream_ptr())
    return gx


def wino43_dgrad_chain_tiles(gy, ud, Cin, tile_list, n_active, out, pool_idx=None, out_gate=None, add_target=None, add_coef=0.0,
                             tile_cols=None):
    """wino43_dgrad_chain over the first n_active (device int32 scalar) tiles of tile_list (device int32), written into
    `out` (N,Cin,H,W) in place: the other tiles of `out` are left alone (st3d_wino43_dgrad_chain_tiles).  tile_cols = 64 /
    32: the list numbers the 4 x 64 / 8 x 32 tiles (st3d_wino43_dgrad_chain_tiles_geo); 16: tile_list holds four strips of 4 x 16
    pixels ((n * H/4 + sy) * W/16 + sx, or -1) of one image per step and n_active counts steps."""
    N, Cout = gy.shape[:2]
    H, W = (2 * gy.shape[2], 2 * gy.shape[3]) if pool_idx is not None else gy.shape[2:]
    assert tuple(out.shape) == (N, Cin, H, W)
    if tile_cols is not None:
        call("st3d_wino43_dgrad_chain_tiles_geo", dptr(gy.contiguous(), F32), dptr(pool_idx, U8), dptr(ud, F32), dptr(out_gate, F32),
             dptr(add_target, F32), float(add_coef), dptr(out, F32), N, Cin, Cout, H, W, int(tile_cols), dptr(tile_list, I32),
             dptr(n_active, I32), stream_ptr())
        return out
    call("st3d_wino43_dgrad_chain_tiles", dptr(gy.contiguous(), F32), dptr(pool_idx, U8), dptr(ud, F32), dptr(out_gate, F32),
         dptr(add_target, F32), float(add_coef), dptr(out, F32), N, Cin, Cout, H, W, dptr(tile_list, I32), dptr(n_active, I32),
         stream_ptr())
    return out


def wino43_fwd_tiles(x, uf, bias, Cout, tile_list, n_active, y=None, yp=None, idx=None, relu=True, tile_cols=None):
    """wino43_fwd over the first n_active (device int32 scalar) tiles of tile_list (device int32), written in place into
    whichever of y (N,Cout,H,W), yp and idx (N,Cout,H/2,W/2) are given; other tiles are left alone (st3d_wino43_fwd_tiles)."""
    N, Cin, H, W = x.shape
    if tile_cols is not None:
        call("st3d_wino43_fwd_tiles_geo", dptr(x.contiguous(), F32), dptr(uf, F32), dptr(bias, F32), dptr(y, F32), dptr(yp, F32),
             dptr(idx, U8), N, Cin, Cout, H, W, 1 if relu else 0, int(tile_cols), dptr(tile_list, I32), dptr(n_active, I32),
             stream_ptr())
        return
    call("st3d_wino43_fwd_tiles", dptr(x.contiguous(), F32), dptr(uf, F32), dptr(bias, F32), dptr(y, F32), dptr(yp, F32),
         dptr(idx, U8), N, Cin, Cout, H, W, 1 if relu else 0, dptr(tile_list, I32), dptr(n_active, I32), stream_ptr())


def wino43_fwd_strips(x, uf, bias, Cout, strip_list, n_steps, y, relu=True):
    """wino43_fwd over the first n_steps (device int32 scalar) steps of strip_list (device int32, four strips of 4 x 16 pixels
    of one image per step, -1 = none), written into y (N,Cout,H,W) in place; nothing else is written (st3d_wino43_fwd_strips)."""
    N, Cin, H, W = x.shape
    assert tuple(y.shape) == (N, Cout, H, W)
    call("st3d_wino43_fwd_strips", dptr(x.contiguous(), F32), dptr(uf, F32), dptr(bias, F32), dptr(y, F32), N, Cin, Cout, H, W,
         1 if relu else 0, dptr(strip_list, I32), dptr(n_steps, I32), stream_ptr())
    return y


def kept_build(cover, first=0, nlists=None, tile_cols=None):
    """cover (N,S,S) uint8 -> {k: (list, count)} for k = first .. nlists - 1: the kept lists of the forward launches conv1_2 ..
    conv3_3 (st3d_kept_build), in the formats of need_blocks_build.  Lists are sized for every tile (strip) and start as -1."""
    lib = _lib.load()
    N, S, _ = cover.shape
    nlists = need_blocks_lists(S) if nlists is None else nlists
    counts = torch.full((6,), -7, dtype=I32, device=cover.device)       # (ST3D_NEED_MAX_LISTS)
    tcols = [int(c or 0) for c in (tile_cols or [0] * nlists)]
    lists = {k: torch.full((lib.st3d_need_blocks_entries(N, S, k, tcols[k]),), -1, dtype=I32, device=cover.device)
             for k in range(first, nlists)}
    nb = lib.st3d_need_blocks_workspace_bytes(N, S)
    ws = torch.empty((max(nb, 1),), dtype=U8, device=cover.device)
    cols = (ctypes.c_int * max(nlists, 1))(*tcols)
    ptrs = (ctypes.c_void_p * max(nlists, 1))(*[lists[k].data_ptr() if k in lists else None for k in range(nlists)])
    call("st3d_kept_build", dptr(cover, U8), N, S, int(first), nlists, cols, dptr(ws), nb, ptrs, dptr(counts), stream_ptr())
    return {k: (lists[k], counts[k]) for k in lists}


def flat_levels(S):
    return _lib.load().st3d_flat_levels(int(S))


def flat_build(imgs, color, levels=None):
    """imgs (N,3,S,S), color (3,) device floats -> [(list, count, map)] for the forward launches of conv1_2, conv2_1 and
    conv2_2 (st3d_flat_build).  Lists and maps are sized for every tile and start as -7; only the first `count` (device
    int32 scalar) list entries are meaningful."""
    N, _, S, _ = imgs.shape
    lib = _lib.load()
    levels = flat_levels(S) if levels is None else levels
    nb = lib.st3d_flat_workspace_bytes(N, S)
    ws = torch.empty((max(nb, 16),), dtype=U8, device=imgs.device)
    counts = torch.full((3,), -7, dtype=I32, device=imgs.device)
    lists = [torch.full((lib.st3d_flat_tiles(N, S, k),), -7, dtype=I32, device=imgs.device) for k in range(levels)]
    maps = [torch.full_like(l, -7) for l in lists]
    ptr = lambda seq, k: dptr(seq[k]) if k < len(seq) else None
    call("st3d_flat_build", dptr(imgs, F32), dptr(color, F32), N, S, levels, dptr(ws), nb, ptr(lists, 0), ptr(maps, 0),
         ptr(lists, 1), ptr(maps, 1), ptr(lists, 2), ptr(maps, 2), dptr(counts), stream_ptr())
    return [(lists[k], counts[k], maps[k]) for k in range(levels)]


def flat_fill(tile_map, y=None, yp=None, idx=None):
    """Every tile with tile_map[t] >= 0 takes the block of tile tile_map[t], in place (st3d_flat_fill)."""
    t = y if y is not None else yp
    N, C = t.shape[:2]
    H, W = (y.shape[2:] if y is not None else (2 * yp.shape[2], 2 * yp.shape[3]))
    call("st3d_flat_fill", dptr(tile_map, I32), dptr(y, F32), dptr(yp, F32), dptr(idx, U8), N, C, H, W, stream_ptr())


def maxpool2x2(y, want_idx=True):
    N, C, H, W = y.shape
    p = torch.empty((N, C, H // 2, W // 2), dtype=F32, device=y.device)
    idx = torch.empty((N, C, H // 2, W // 2), dtype=U8, device=y.device) if want_idx else None
    call("st3d_maxpool2x2_fwd", dptr(y.contiguous(), F32), dptr(p), dptr(idx), N, C, H, W, stream_ptr())
    return (p, idx) if want_idx else p


# ------------------------------------------------------------------ gram / losses
GUIDANCE_LEVELS = 5


def guidance_sides(S):
    """sides of the five guidance planes: the style taps' (each pool floors)"""
    return [S >> l for l in range(GUIDANCE_LEVELS)]


def _guidance_mask(mask):
    """(n,1,S,S) or (n,S,S) fp32 device tensor -> contiguous (n,S,S)"""
    if not torch.is_tensor(mask):
        raise _lib.St3dError("the guidance mask is a tensor (n,1,S,S) or (n,S,S)")
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 3 or mask.shape[1] != mask.shape[2] or mask.shape[0] < 1 or mask.shape[1] < 16:
        raise _lib.St3dError(f"the guidance mask is (n,1,S,S) or (n,S,S) with S >= 16; got {tuple(mask.shape)}")
    if not mask.is_cuda:
        raise _lib.St3dError("libst3d takes device tensors; got a CPU mask (no CPU fallback)")
    if mask.dtype != F32:
        raise _lib.St3dError(f"expected {F32}, got {mask.dtype}")
    return mask.detach().contiguous()


def guidance_build(mask):
    """mask (n,1,S,S) | (n,S,S) in [0,1] -> (planes, sums): planes[l] (n,H_l,H_l) = q_l = sqrt(a_l H_l^2 / Sigma_l) with a_l
    the 2x2 average pyramid of the mask (views of one buffer), sums (5,n) = Sigma_l (st3d_guidance_build)."""
    m = _guidance_mask(mask)
    n, S = m.shape[0], m.shape[1]
    lib = _lib.load()
    q = torch.empty((lib.st3d_guidance_floats(n, S),), dtype=F32, device=m.device)
    sums = torch.empty((GUIDANCE_LEVELS, n), dtype=F32, device=m.device)
    parts = torch.empty((lib.st3d_guidance_partials(n, S),), dtype=F32, device=m.device)
    call("st3d_guidance_build", dptr(m, F32), n, S, dptr(q), dptr(sums), dptr(parts), stream_ptr())
    planes, off = [], 0
    for H in guidance_sides(S):
        planes.append(q[off:off + n * H * H].view(n, H, H))
        off += n * H * H
    return planes, sums


def _check_q(q, B, HW):
    if q.numel() != B * HW:
        raise _lib.St3dError(f"the weight plane has {q.numel()} values, the features {B} x {HW} pixels")
    return dptr(q.contiguous(), F32)


def gram_fwd(feat, q=None):
    """(B,C,H,W) or (B,C,HW) -> (B,C,C) unnormalised Gram (style_transfer.py:31-35).  q (B,H,W) | (B,HW): the guided Gram
    sum_p q[p]^2 F[:,p] F[:,p]^T (st3d_gram_fwd_weighted; q from guidance_build)."""
    B, C = feat.shape[:2]
    HW = feat[0, 0].numel()
    ws_bytes = _lib.load().st3d_gram_workspace_bytes(B, C, HW)
    ws = torch.empty((max(ws_bytes // 4, 1),), dtype=F32, device=feat.device)
    g = torch.empty((B, C, C), dtype=F32, device=feat.device)
    if q is None:
        call("st3d_gram_fwd", dptr(feat.contiguous(), F32), B, C, HW, dptr(ws), ws_bytes, dptr(g), stream_ptr())
    else:
        call("st3d_gram_fwd_weighted", dptr(feat.contiguous(), F32), _check_q(q, B, HW), B, C, HW, dptr(ws), ws_bytes, dptr(g),
             stream_ptr())
    return g


class _GramItem(ctypes.Structure):
    _fields_ = [("feat", ctypes.c_void_p), ("gram", ctypes.c_void_p), ("B", ctypes.c_int), ("C", ctypes.c_int), ("HW", ctypes.c_int)]


def gram_fwd_multi(feats, qs=None):
    """[(B,C,H,W) ...] -> [(B,C,C) ...]: the Grams of several layers in one launch pair (st3d_gram_fwd_multi); qs: one
    weight plane per layer (st3d_gram_fwd_multi_weighted)."""
    feats = [f.contiguous() for f in feats]
    grams = [torch.empty((f.shape[0], f.shape[1], f.shape[1]), dtype=F32, device=f.device) for f in feats]
    items = (_GramItem * len(feats))()
    for it, f, g in zip(items, feats, grams):
        it.feat, it.gram, it.B, it.C, it.HW = dptr(f, F32), dptr(g, F32), f.shape[0], f.shape[1], f[0, 0].numel()
    nb = _lib.load().st3d_gram_multi_workspace_bytes(items, len(feats))
    ws = torch.empty((max(nb // 4, 64),), dtype=F32, device=feats[0].device)
    assert ws.data_ptr() % 256 == 0
    if qs is None:
        call("st3d_gram_fwd_multi", items, len(feats), dptr(ws), nb, stream_ptr())
    else:
        if len(qs) != len(feats):
            raise _lib.St3dError("one weight plane per layer")
        qs = [q.contiguous() for q in qs]
        qp = (ctypes.c_void_p * len(feats))(*[_check_q(q, f.shape[0], f[0, 0].numel()) for q, f in zip(qs, feats)])
        call("st3d_gram_fwd_multi_weighted", items, qp, len(feats), dptr(ws), nb, stream_ptr())
    return grams


def gram_bwd(D, feat, coef, out=None, gated=False, q=None):
    """out (+)= coef * D feat; gated: then zeroed where feat <= 0 (st3d_gram_bwd_gated).  q: the guided term's gradient
    out (+)= coef * q (D (q feat)) (st3d_gram_bwd_weighted)."""
    B, C = feat.shape[:2]
    HW = feat[0, 0].numel()
    acc = 1
    if out is None:
        out = torch.empty_like(feat)
        acc = 0
    if q is not None:
        call("st3d_gram_bwd_weighted", dptr(D.contiguous(), F32), dptr(feat.contiguous(), F32), _check_q(q, B, HW), B, C, HW,
             float(coef), acc, 1 if gated else 0, dptr(out), stream_ptr())
        return out
    call("st3d_gram_bwd_gated" if gated else "st3d_gram_bwd", dptr(D.contiguous(), F32), dptr(feat.contiguous(), F32), B, C, HW, float(coef), acc, dptr(out),
         stream_ptr())
    return out


def sqdiff_sum(a, b, scale=1.0, want_diff=False):
    n, nb = a.numel(), b.numel()
    parts = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=a.device)
    out = torch.zeros((1,), dtype=F32, device=a.device)
    D = torch.empty_like(a) if want_diff else None
    call("st3d_sqdiff_sum", dptr(a.contiguous(), F32), dptr(b.contiguous(), F32), n, nb, float(scale), dptr(D),
         dptr(parts), dptr(out), stream_ptr())
    return (out, D) if want_diff else out


class _SqdiffItem(ctypes.Structure):
    _fields_ = [("a", ctypes.c_void_p), ("b", ctypes.c_void_p), ("D", ctypes.c_void_p), ("n", ctypes.c_size_t),
                ("nb", ctypes.c_size_t), ("scale", ctypes.c_float), ("slot", ctypes.c_int)]


def sqdiff_sum_multi(items, zero_first, combine, style_weight, content_weight, out=None):
    """Up to 8 squared-difference sums in one launch pair (st3d_sqdiff_sum_multi).  items: (a, b, scale, slot, want_diff)
    each; b is broadcast when it is shorter (a.numel() % b.numel() == 0).  Item k adds scale * sum((a - b)^2) into
    out[slot]; zero_first clears the three slots first; combine then sets out[0] = content_weight * out[1] +
    style_weight * out[2].  -> (out (3,) [total, content, style], [D or None per item])."""
    if not 0 < len(items) <= 8:
        raise ValueError("st3d_sqdiff_sum_multi takes 1 to 8 items")
    dev = items[0][0].device
    if out is None:
        out = torch.zeros((3,), dtype=F32, device=dev)
    arr = (_SqdiffItem * len(items))()
    keep, diffs = [], []
    for it, (a, b, scale, slot, want_diff) in zip(arr, items):
        a, b = a.contiguous(), b.contiguous()
        D = torch.empty_like(a) if want_diff else None
        keep += [a, b]
        diffs.append(D)
        it.a, it.b, it.D = dptr(a, F32), dptr(b, F32), dptr(D)
        it.n, it.nb, it.scale, it.slot = a.numel(), b.numel(), float(scale), int(slot)
    parts = torch.empty((len(items) * _lib.load().st3d_reduce_partials(),), dtype=F32, device=dev)
    call("st3d_sqdiff_sum_multi", arr, len(items), dptr(parts), dptr(out, F32), 1 if zero_first else 0, 1 if combine else 0,
         float(style_weight), float(content_weight), stream_ptr())
    return out, diffs


def masked_mse(rendered, target, mask, want_grad=True):
    B, _, S, _ = rendered.shape
    parts = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=rendered.device)
    out = torch.zeros((1,), dtype=F32, device=rendered.device)
    g = torch.empty_like(rendered) if want_grad else None
    call("st3d_masked_mse", dptr(rendered.contiguous(), F32), dptr(target.contiguous(), F32), dptr(mask.contiguous(), F32),
         B, S, dptr(g), dptr(parts), dptr(out), stream_ptr())
    return out, g


def tv_loss(images, masks, want_grad=True):
    """masked anisotropic L1 TV / sum(masks) -> (loss (1,), grad_images | None)"""
    B, C, H, W = images.shape
    parts = torch.empty((2 * _lib.load().st3d_reduce_partials(),), dtype=F32, device=images.device)
    out = torch.zeros((2,), dtype=F32, device=images.device)
    g = torch.empty_like(images, memory_format=torch.contiguous_format) if want_grad else None
    call("st3d_tv_loss", dptr(images.contiguous(), F32), dptr(masks.contiguous(), F32), B, C, H, W, dptr(parts), dptr(out),
         dptr(g), stream_ptr())
    return out[:1], g


def range_loss(values, want_grad=True):
    """sum relu(v - 1) + relu(-v) -> (loss (1,), grad | None)"""
    v = values.contiguous()
    parts = torch.empty((_lib.load().st3d_reduce_partials(),), dtype=F32, device=v.device)
    out = torch.zeros((1,), dtype=F32, device=v.device)
    g = torch.empty_like(v) if want_grad else None
    call("st3d_range_loss", dptr(v, F32), v.numel(), dptr(parts), dptr(out), dptr(g), stream_ptr())
    return out, g


# ------------------------------------------------------------------ texture pyramid (csrc/texpyr.hip)
def texpyr_sides(T, levels):
    """Sides [T, T/2, ...] of a pyramid of `levels` maps under a T x T texture.  levels = 0 is "auto": halve while the side
    is even and the half is >= 4 (512 -> 8 levels down to 4, 768 -> 8 down to 6).  levels >= 2 needs T divisible by
    2^(levels-1) and a coarsest side >= 2.  Pure host logic; anything else raises ValueError."""
    T, levels = int(T), int(levels)
    if T < 1:
        raise ValueError(f"texture side must be positive, got {T}")
    if levels < 0:
        raise ValueError(f"texture pyramid levels must be >= 0 (0 = auto), got {levels}")
    if levels == 0:
        sides = [T]
        while sides[-1] % 2 == 0 and sides[-1] // 2 >= 4:
            sides.append(sides[-1] // 2)
        return sides
    if levels > 16:
        raise ValueError(f"at most 16 texture pyramid levels, got {levels}")
    if levels > 1 and (T % (1 << (levels - 1)) or T >> (levels - 1) < 2):
        raise ValueError(f"{levels} pyramid levels need a texture side divisible by {1 << (levels - 1)} with a coarsest side "
                         f">= 2, got {T}")
    return [T >> l for l in range(levels)]


def texpyr_numel(T, L):
    """P = 3 * sum_l (T / 2^l)^2, the length of the flat parameter tensor of an L-level pyramid (L >= 1)."""
    if int(L) < 1:
        raise ValueError(f"texpyr_numel takes a resolved level count >= 1 (see texpyr_sides), got {L}")
    texpyr_sides(T, L)
    n = _lib.load().st3d_texpyr_numel(int(T), int(L))
    if n == 0:
        raise ValueError(f"no texture pyramid of {L} levels under a side of {T}")
    return n


def texpyr_synth(params, T, L, out=None):
    """flat params (P,) -> texture (1,T,T,3) = level_0 + up2(level_1 + up2(...)); one launch whatever L is."""
    P = texpyr_numel(T, L)
    if params.numel() != P:
        raise ValueError(f"a {L}-level pyramid under side {T} holds {P} values, got {params.numel()}")
    if out is None:
        out = torch.empty((1, T, T, 3), dtype=F32, device=params.device)
    call("st3d_texpyr_synth", dptr(params, F32), int(T), int(L), dptr(out, F32), stream_ptr())
    return out


def texpyr_adjoint(grad_texture, T, L, out=None):
    """grad_texture (T*T*3 values, HWC) -> the gradient of the flat params (P,): every coarse texel gathers its fine
    footprint in a fixed order (no atomics); at most two launches."""
    P = texpyr_numel(T, L)
    if grad_texture.numel() != 3 * T * T:
        raise ValueError(f"grad_texture must hold {T}x{T}x3 values, got {tuple(grad_texture.shape)}")
    if out is None:
        out = torch.empty((P,), dtype=F32, device=grad_texture.device)
    call("st3d_texpyr_adjoint", dptr(grad_texture.contiguous(), F32), int(T), int(L), dptr(out, F32), stream_ptr())
    return out


# ------------------------------------------------------------------ image pyramid step (csrc/imgpyr.hip)
# The device wrappers live in st3d/imgpyr.py, next to the autograd function and the caches built on them (as st3d/fill.py
# holds those of fill.hip); they are re-exported here so that ops keeps one name per entry point of include/st3d.h.
from .imgpyr import pyr_down_bwd, pyr_down_fwd, pyr_down_need, pyr_down_tile  # noqa: E402,F401


# ------------------------------------------------------------------ colour control (csrc/color.hip)
# As above: the device wrappers live in st3d/color.py next to the autograd function, the cache and the host-side match.
# st3d_color_stats is ``color_sums`` here as there (the ten sums on the device): ``color_stats`` is the name of the public
# function of st3d.color that returns mean and covariance, and one name does not get two return types.
from .color import color_affine, color_stats_chunk, color_sums, luma_bwd, luma_fwd, luma_recombine  # noqa: E402,F401


# ------------------------------------------------------------------ Laplacian content term (csrc/lap.hip)
# As above: the device wrappers live in st3d/lap.py next to the pool checks and the target cache.
from .lap import lap_fwd, lap_loss, lap_tile  # noqa: E402,F401


# ------------------------------------------------------------------ mip-mapped sampling (csrc/mipmap.hip)
MIP_MAX_LEVELS = 16


def check_mip(levels, T=None):
    """texture_mip_levels -> the resolved level count L >= 1 under a T x T map (ValueError otherwise).  0 = the full chain:
    the largest L with T divisible by 2^(L-1) and a coarsest side >= 2 (64 -> 6, 48 -> 5, 37 -> 1); 1 = off; L >= 2 needs
    exactly that of T.  Without T only the value itself is checked and returned."""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 0 <= levels <= MIP_MAX_LEVELS:
        raise ValueError(f"texture_mip_levels must be an int in 0..{MIP_MAX_LEVELS} (0 = full chain, 1 = off), got {levels!r}")
    if T is None:
        return levels
    T = int(T)
    if T < 2:
        raise ValueError(f"mip-mapping needs a texture side >= 2, got {T}")
    if levels == 0:
        L = 1
        while L < MIP_MAX_LEVELS and T % (1 << L) == 0 and T >> L >= 2:
            L += 1
        return L
    if levels > 1 and (T % (1 << (levels - 1)) or T >> (levels - 1) < 2):
        raise ValueError(f"texture_mip_levels = {levels} needs a texture side divisible by {1 << (levels - 1)} with a coarsest "
                         f"side >= 2, got {T}")
    return levels


def check_lod_bias(bias):
    bias = float(bias)
    if not math.isfinite(bias):
        raise ValueError(f"texture_lod_bias must be finite, got {bias!r}")
    return bias


def mip_numel(T, L):
    """3 * sum_l (T >> l)^2: the length of the packed mip chain (the texture pyramid's layout) of L >= 1 levels."""
    L = check_mip(int(L), T)
    n = _lib.load().st3d_mip_numel(int(T), L)
    if n == 0:
        raise ValueError(f"no mip chain of {L} levels under a side of {T}")
    return n


def mip_build(texture, L, out=None):
    """texture (T*T*3 values, HWC) -> packed chain (P,): level_{l+1} = 2 x 2 box mean of level_l, ((a + b) + (c + d)) * 0.25"""
    T = texture.shape[-2]
    P = mip_numel(T, L)
    if texture.numel() != 3 * T * T:
        raise ValueError(f"texture must hold {T}x{T}x3 values, got {tuple(texture.shape)}")
    if out is None:
        out = torch.empty((P,), dtype=F32, device=texture.device)
    call("st3d_mip_build", dptr(texture.contiguous(), F32), int(T), int(L), dptr(out, F32), stream_ptr())
    return out


def mip_adjoint(grad_pyramid, T, L, out=None):
    """packed per-level gradient (P,) -> (T,T,3): the adjoint of mip_build, folded coarse to fine in a fixed order.  `out`:
    an existing gradient the result is ADDED to."""
    P = mip_numel(T, L)
    if grad_pyramid.numel() != P:
        raise ValueError(f"a {L}-level chain under side {T} holds {P} values, got {grad_pyramid.numel()}")
    acc = 1
    if out is None:
        out = torch.empty((T, T, 3), dtype=F32, device=grad_pyramid.device)
        acc = 0
    call("st3d_mip_adjoint", dptr(grad_pyramid.contiguous(), F32), int(T), int(L), acc, dptr(out, F32), stream_ptr())
    return out


def mip_lod(frag, verts_ndc, faces_i32, verts_uvs, faces_uvs_i32, T, L, bias=0.0):
    """-> lod (B,S,S): the level of detail lambda in [0, L-1] of every covered pixel (0 elsewhere), analytic per fragment"""
    p2f, zbuf, bary, _dists = frag
    B, S, _ = p2f.shape
    L, bias = check_mip(int(L), T), check_lod_bias(bias)
    lod = torch.empty((B, S, S), dtype=F32, device=p2f.device)
    call("st3d_mip_lod", dptr(p2f, I32), dptr(bary, F32), dptr(zbuf, F32), dptr(verts_ndc, F32), dptr(faces_i32, I32),
         dptr(verts_uvs, F32), dptr(faces_uvs_i32, I32), B, S, int(T), L, verts_ndc.shape[1], faces_i32.shape[0],
         verts_uvs.shape[0], bias, dptr(lod), stream_ptr())
    return lod


def _mip_check_planes(p2f, pyramid, lod, T, L):
    P = mip_numel(T, L)
    if pyramid.numel() != P:
        raise ValueError(f"a {L}-level chain under side {T} holds {P} values, got {pyramid.numel()}")
    if tuple(lod.shape) != tuple(p2f.shape):
        raise ValueError(f"lod must be {tuple(p2f.shape)}, got {tuple(lod.shape)}")


def shade_mip_fwd(frag, verts_uvs, faces_uvs_i32, pyramid, lod, T, L):
    """shade_fwd sampling the packed chain trilinearly at lod -> rgb (B,3,S,S), mask (B,1,S,S)"""
    p2f = frag[0]
    B, S, _ = p2f.shape
    _mip_check_planes(p2f, pyramid, lod, T, L)
    rgb, mask = _rgb_mask(B, S, p2f.device)
    call("st3d_shade_mip_fwd", *_frag_head(frag), *_uv_head(verts_uvs, faces_uvs_i32, pyramid), dptr(lod, F32), B, S, int(T),
         int(L), faces_uvs_i32.shape[0], verts_uvs.shape[0], dptr(rgb), dptr(mask), stream_ptr())
    return rgb, mask


def shade_mip_bwd(grad_rgb, frag, verts_uvs, faces_uvs_i32, pyramid, lod, T, L, grad_texture=None, want_uv=False,
                  want_bary=False, want_texture=True, want_levels=False):
    """-> grad_texture (T,T,3) [, grad_uv (B,S,S,2)] [, grad_bary (B,S,S,3)] [, the per-level gradient (P,) before the
    fold]; lod is a constant.  Fixed point (bitwise reproducible) unless set_deterministic(False)."""
    p2f = frag[0]
    B, S, _ = p2f.shape
    dev = p2f.device
    _mip_check_planes(p2f, pyramid, lod, T, L)
    if tuple(grad_rgb.shape) != (B, 3, S, S):
        raise ValueError(f"grad_rgb must be {(B, 3, S, S)}, got {tuple(grad_rgb.shape)}")
    if grad_texture is None and want_texture:
        grad_texture = torch.zeros((T, T, 3), dtype=F32, device=dev)
    gpyr = torch.empty((pyramid.numel(),), dtype=F32, device=dev) if grad_texture is not None else None
    guv = torch.empty((B, S, S, 2), dtype=F32, device=dev) if want_uv else None
    gbary = torch.empty((B, S, S, 3), dtype=F32, device=dev) if want_bary else None
    ws, nb = (_det_ws(_lib.load().st3d_shade_mip_bwd_workspace_bytes(int(T), int(L)), dev)
              if _DETERMINISTIC and grad_texture is not None else (None, 0))
    call("st3d_shade_mip_bwd", dptr(grad_rgb.contiguous(), F32), *_frag_head(frag),
         *_uv_head(verts_uvs, faces_uvs_i32, pyramid), dptr(lod, F32), B, S, int(T), int(L), faces_uvs_i32.shape[0],
         verts_uvs.shape[0], dptr(gpyr), dptr(grad_texture, F32), dptr(guv), dptr(gbary), dptr(ws), nb, stream_ptr())
    return _outputs(grad_texture, (want_uv, guv), (want_bary, gbary), (want_levels, gpyr))


def adam_step(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    call("st3d_adam_step", dptr(p, F32), dptr(g.contiguous(), F32), dptr(m, F32), dptr(v, F32), p.numel(), int(step),
         float(lr), float(b1), float(b2), float(eps), stream_ptr())


def device_info(device=0):
    cu = ctypes.c_int(0)
    hbm = ctypes.c_size_t(0)
    name = ctypes.create_string_buffer(128)
    call("st3d_device_info", device, ctypes.byref(cu), ctypes.byref(hbm), name, 128)
    return {"cu_count": cu.value, "hbm_bytes": hbm.value, "name": name.value.decode()}



# ---------------------------------------------------------------------------- roctx ranges (ST3D_ROCTX=1; include/st3d.h)
class trace:
    """with ops.trace("render"): ...  -- a named range for rocprofv3 --marker-trace around a host phase of the step (the
    library marks the VGG phases itself).  Costs nothing unless ST3D_ROCTX=1 was set before the first call."""
    _on = None

    def __init__(self, name):
        self.name = name.encode()

    def __enter__(self):
        if trace._on is None:
            trace._on = os.environ.get("ST3D_ROCTX") == "1" and _lib.load().st3d_trace_enabled() == 1
        if trace._on:
            _lib.load().st3d_trace_push(self.name)
        return self

    def __exit__(self, *exc):
        if trace._on:
            _lib.load().st3d_trace_pop()
        return False
