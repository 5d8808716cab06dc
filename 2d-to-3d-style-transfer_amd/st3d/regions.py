"""Style regions (--style_regions): one style image per region of the mesh.

A region is a set of faces: one integer label 0..R-1 per face, R <= 8, from the OBJ's ``usemtl`` groups, from cuts along an
axis, or from a ``.npy`` file.  Per-face labels are view-consistent by construction, so the guidance of every view follows
from the fragments of its own render: ``region_planes`` takes ``pix_to_face`` and the labels to the guidance planes of all
regions in one launch pair (csrc/regions.hip: region r's planes are bit for bit ``ops.guidance_build`` of its one-hot
mask; background pixels belong to no region).  ``region_targets`` holds one plain Gram per region's style image and tap.
The loss over them is ``style_transfer.region_style_loss`` / ``losses.compute_region_style_loss``."""
import os

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, dptr, stream_ptr

MAX_REGIONS = 8
F32, I32, U8 = torch.float32, torch.int32, torch.uint8

# the debug preview's colours, region 0..7 (background: white)
PALETTE = ((0.90, 0.10, 0.10), (0.10, 0.45, 0.90), (0.15, 0.70, 0.20), (0.95, 0.75, 0.10),
           (0.60, 0.20, 0.80), (0.10, 0.75, 0.75), (0.95, 0.45, 0.10), (0.45, 0.45, 0.45))


# ------------------------------------------------------------------------------------------------ labels (host)
def check_face_regions(labels, F, device=None):
    """labels: F integers in 0..R-1 with every label present and R <= 8 -> (uint8 tensor (F,) on ``device`` -- default the
    labels' own device if they are a device tensor, else the current GPU --, R); anything else: ValueError.  The one place
    labels are validated: the kernel cannot, and the check reads them back once per run."""
    if torch.is_tensor(labels):
        if device is None and labels.is_cuda:
            device = labels.device
        arr = labels.detach().cpu().numpy()
    else:
        arr = np.asarray(labels)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"face regions must be integers, got {arr.dtype}")
    if isinstance(F, bool) or not isinstance(F, int) or F < 1:
        raise ValueError(f"the face count must be a positive integer, got {F!r}")
    if arr.shape != (F,):
        raise ValueError(f"face regions must have shape ({F},), one label per face; got {arr.shape}")
    lo, hi = int(arr.min()), int(arr.max())
    if lo < 0:
        raise ValueError(f"face regions must be >= 0, got {lo}")
    R = hi + 1
    if R > MAX_REGIONS:
        raise ValueError(f"at most {MAX_REGIONS} regions, got labels up to {hi}")
    present = np.bincount(arr.astype(np.int64), minlength=R)
    if (present == 0).any():
        raise ValueError(f"every label 0..{R - 1} must name at least one face; {int(np.flatnonzero(present == 0)[0])} names none")
    t = torch.from_numpy(arr.astype(np.uint8))
    return t.to(device if device is not None else "cuda").contiguous(), R


def regions_from_materials(materials_idx):
    """``st3d.io.load_obj(...)[1].materials_idx`` (F,) -> int64 numpy labels (F,): the OBJ's ``usemtl`` groups numbered by
    first appearance in face order (faces in front of the first ``usemtl`` are a group of their own)."""
    m = materials_idx.detach().cpu().numpy() if torch.is_tensor(materials_idx) else np.asarray(materials_idx)
    if m.ndim != 1 or m.size == 0:
        raise ValueError(f"materials_idx must be (F,) with F >= 1, got shape {m.shape}")
    _, first, inverse = np.unique(m, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)]


def count_material_groups(obj_path):
    """how many regions 'material' would give for this OBJ, from its ``usemtl`` and ``f`` lines alone (what the parser can
    know before the mesh is loaded): the distinct materials that at least one face uses, faces in front of the first
    ``usemtl`` counting as one more"""
    used, cur = set(), None
    with open(obj_path, "r") as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "usemtl" and len(tok) > 1:
                cur = tok[1]
            elif tok[0] == "f":
                used.add(cur)
    return len(used)


AXES = {"x": 0, "y": 1, "z": 2}


def check_cuts(cuts):
    """k >= 1 finite, strictly increasing cuts with k + 1 <= 8 -> tuple of floats; else ValueError"""
    try:
        cuts = tuple(float(c) for c in cuts)
    except (TypeError, ValueError):
        raise ValueError(f"cuts must be numbers, got {cuts!r}") from None
    if not cuts or not all(np.isfinite(cuts)):
        raise ValueError(f"cuts must be one or more finite numbers, got {cuts!r}")
    if any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cuts must be strictly increasing, got {cuts!r}")
    if len(cuts) + 1 > MAX_REGIONS:
        raise ValueError(f"{len(cuts)} cuts make {len(cuts) + 1} regions; at most {MAX_REGIONS}")
    return cuts


def regions_from_axis(verts, faces, axis, cuts):
    """Faces split by the centroid of the mesh AS LOADED along ``axis`` ('x' | 'y' | 'z'): k strictly increasing cuts give
    k + 1 slabs, slab = the number of cuts the centroid coordinate is strictly greater than (a centroid exactly on a cut
    stays below it).  The centroid is the fp64 mean of the three fp32 corners.  -> int64 numpy labels (F,).  A slab
    without a face is the caller's to refuse (labels_from_spec does)."""
    if axis not in AXES:
        raise ValueError(f"axis must be one of x, y, z; got {axis!r}")
    cuts = check_cuts(cuts)
    v = (verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)).astype(np.float64)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"verts must be (V,3) and faces (F,3), got {v.shape} and {f.shape}")
    c = v[f, AXES[axis]]
    c = ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0
    return np.searchsorted(np.asarray(cuts, dtype=np.float64), c, side="left").astype(np.int64)


def load_face_regions(path):
    """a ``.npy`` integer array of shape (F,) -> int64 numpy labels; else ValueError"""
    arr = np.load(path, allow_pickle=False)
    if arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer) or arr.ndim != 1:
        raise ValueError(f"{path}: face regions are a one-dimensional integer array, got {arr.dtype} {arr.shape}")
    return arr.astype(np.int64)


def parse_spec(spec):
    """--style_regions SPEC -> ('material',) | ('axis', 'x'|'y'|'z', cuts) | ('file', path); else ValueError"""
    if not isinstance(spec, str) or not spec:
        raise ValueError("the regions are 'material', an axis with cuts such as x:0 or y:-0.1,0.2, or a .npy file")
    if spec == "material":
        return ("material",)
    if len(spec) >= 2 and spec[0] in AXES and spec[1] == ":":
        try:
            cuts = [float(c) for c in spec[2:].split(",")]
        except ValueError:
            raise ValueError(f"the cuts of {spec!r} must be numbers: axis:c[,c...]") from None
        return ("axis", spec[0], check_cuts(cuts))
    if spec.endswith(".npy"):
        return ("file", spec)
    raise ValueError(f"the regions are 'material', an axis with cuts such as x:0 or y:-0.1,0.2, or a .npy file; got {spec!r}")


def labels_from_spec(spec, verts, faces, materials_idx=None):
    """the int64 numpy labels (F,) ``spec`` (a string or its ``parse_spec``) gives on the loaded mesh; not yet validated"""
    parsed = parse_spec(spec) if isinstance(spec, str) else spec
    if parsed[0] == "material":
        if materials_idx is None or len(materials_idx) != len(faces):
            raise ValueError("the mesh carries no material index per face: 'material' regions need an OBJ with usemtl groups")
        labels = regions_from_materials(materials_idx)
        if int(labels.max()) + 1 < 2:
            raise ValueError("'material' regions need an OBJ with at least 2 usemtl groups; this one has 1, so the regions "
                             "would be the whole object (--style_mask object does that)")
        return labels
    if parsed[0] == "axis":
        labels = regions_from_axis(verts, faces, parsed[1], parsed[2])
        count = np.bincount(labels, minlength=len(parsed[2]) + 1)
        if (count == 0).any():
            raise ValueError(f"slab {int(np.flatnonzero(count == 0)[0])} of {parsed[1]}:{','.join(f'{c:g}' for c in parsed[2])} "
                             "holds no face of this mesh: every region needs at least one")
        return labels
    if not os.path.isfile(parsed[1]):
        raise ValueError(f"no such file: {parsed[1]}")
    return load_face_regions(parsed[1])


# ------------------------------------------------------------------------------------------------ planes (device)
def _check_fragments(pix_to_face):
    if not torch.is_tensor(pix_to_face):
        raise _lib.St3dError("pix_to_face is a tensor (n,S,S)")
    if not pix_to_face.is_cuda:
        raise _lib.St3dError("libst3d takes device tensors; got CPU fragments (no CPU fallback)")
    p = pix_to_face
    if p.dim() == 4 and p.shape[3] == 1:
        p = p[..., 0]
    if p.dim() != 3 or p.shape[1] != p.shape[2] or p.shape[0] < 1 or p.shape[1] < 16:
        raise _lib.St3dError(f"pix_to_face is (n,S,S) of a one-face-per-pixel render with S >= 16; got {tuple(pix_to_face.shape)}")
    if p.dtype != I32:
        raise _lib.St3dError(f"expected {I32}, got {p.dtype}")
    return p.contiguous()


def _check_labels(face_regions, R):
    if not torch.is_tensor(face_regions) or face_regions.dtype != U8 or face_regions.dim() != 1 or not face_regions.is_cuda:
        raise _lib.St3dError("face_regions is the uint8 device tensor (F,) of check_face_regions")
    if isinstance(R, bool) or not isinstance(R, int) or not 1 <= R <= MAX_REGIONS:
        raise _lib.St3dError(f"R must be an integer in 1..{MAX_REGIONS}, got {R!r}")
    return face_regions.contiguous()


def region_planes(pix_to_face, face_regions, R):
    """pix_to_face (n,S,S) int32 (< 0: no face; every index < F, the rasteriser's guarantee), face_regions the validated
    uint8 labels (F,), R -> (planes, sums): planes[r][l] (n,H_l,H_l) = region r's q_l (views of one buffer, each region's
    block laid out as ops.guidance_build's), sums (R,5,n) = Sigma_l (st3d_region_planes)."""
    p = _check_fragments(pix_to_face)
    lab = _check_labels(face_regions, R)
    n, S = p.shape[0], p.shape[1]
    lib = _lib.load()
    per = lib.st3d_guidance_floats(n, S)
    q = torch.empty((lib.st3d_region_planes_floats(n, S, R),), dtype=F32, device=p.device)
    sums = torch.empty((R, ops.GUIDANCE_LEVELS, n), dtype=F32, device=p.device)
    parts = torch.empty((lib.st3d_region_planes_partials(n, S, R),), dtype=F32, device=p.device)
    call("st3d_region_planes", dptr(p, I32), dptr(lab, U8), n, S, lab.shape[0], R, dptr(q), dptr(sums), dptr(parts), stream_ptr())
    planes = []
    for r in range(R):
        off, mine = r * per, []
        for H in ops.guidance_sides(S):
            mine.append(q[off:off + n * H * H].view(n, H, H))
            off += n * H * H
        planes.append(mine)
    return planes, sums


def fragments_of(rendered):
    """The pix_to_face (n,S,S) behind a colour tensor a hard one-face-per-pixel render returned (or its composite onto a
    background): the fragments its own backward keeps -- the rasteriser's FragmentCache entry when the view came from it --,
    so nothing is rasterised a second time.  None when the tensor carries no such fragments."""
    node = getattr(rendered, "grad_fn", None)
    for _ in range(2):                              # the render itself, or one composite in front of it
        if node is None:
            return None
        frag = getattr(node, "frag", None)
        if frag is not None:
            p = frag[0]
            if torch.is_tensor(p) and p.dim() == 4 and p.shape[3] == 1:     # the general kernels at one face per pixel
                p = p[..., 0]
            return p if torch.is_tensor(p) and p.dim() == 3 and p.dtype == I32 else None
        nxt = getattr(node, "next_functions", ())
        node = nxt[0][0] if nxt else None
    return None


def region_preview(pix_to_face, face_regions):
    """(n,3,S,S) in [0,1]: every covered pixel in its region's colour of PALETTE, the background white (a debug picture:
    plain torch indexing)."""
    p = _check_fragments(pix_to_face).long()
    lab = face_regions.to(p.device).long()
    pal = torch.tensor(PALETTE + ((1.0, 1.0, 1.0),), dtype=F32, device=p.device)
    idx = torch.where(p >= 0, lab[p.clamp_min(0)].clamp_max(MAX_REGIONS - 1), torch.full_like(p, MAX_REGIONS))
    return pal[idx].permute(0, 3, 1, 2).contiguous()


def region_shares(sums):
    """sums (R,5,n) of one or more view batches (a tensor or a list of them) -> R floats: each region's share of the covered
    pixels over all views (level 0 counts pixels exactly)."""
    batches = [sums] if torch.is_tensor(sums) else list(sums)
    per = torch.stack([s[:, 0, :].double().sum(dim=1).cpu() for s in batches]).sum(dim=0)
    total = float(per.sum())
    return [float(v) / total if total > 0 else 0.0 for v in per]


# ------------------------------------------------------------------------------------------------ targets
def region_targets(style_imgs, model):
    """style_imgs (R,3,S,S): one style image per region, at the side of the renders -> A[r][l] (1,C_l,C_l): the plain
    unweighted Grams of each image's five style taps.  Computed once: cached on the model under the tensor's identity and
    version, as the plan caches set_style's."""
    import style_transfer as _st
    if not torch.is_tensor(style_imgs) or style_imgs.dim() != 4 or style_imgs.shape[1] != 3 \
            or style_imgs.shape[2] != style_imgs.shape[3] or not 1 <= style_imgs.shape[0] <= MAX_REGIONS:
        raise ValueError(f"style_imgs must be (R,3,S,S) with R in 1..{MAX_REGIONS}, one image per region; got "
                         f"{tuple(getattr(style_imgs, 'shape', ()))}")
    if not style_imgs.is_cuda:
        raise RuntimeError("st3d runs on the GPU (libst3d); got CPU style images -- there is no CPU fallback")
    key = (style_imgs.data_ptr(), style_imgs._version, tuple(style_imgs.shape), tuple(style_imgs.stride()))
    cache = getattr(model, "_region_target_cache", None)
    if cache is not None and cache[0] == key and cache[1].data_ptr() == style_imgs.data_ptr():
        return cache[2]
    with torch.no_grad():
        feats = _st.get_features(style_imgs.detach().to(F32).contiguous(), model, _st.REGION_STYLE_TAPS)
        grams = ops.gram_fwd_multi([feats[name] for name in _st.REGION_STYLE_TAPS.values()])
    targets = [[g[r:r + 1].contiguous() for g in grams] for r in range(style_imgs.shape[0])]
    model._region_target_cache = (key, style_imgs, targets)
    return targets
