"""Host-side asset I/O: Wavefront OBJ/MTL + texture image load, OBJ/MTL/PNG save.

Replaces what the reference gets from ``pytorch3d.io.load_obj`` / ``IO().save_mesh``
(first_approach.py:83-88,225; second_approach.py:77-82,202) -- semantics per SURVEY.md A.5:
1-based (or negative = relative) indices, ``f`` tokens ``v``, ``v/vt``, ``v//vn``,
``v/vt/vn``, polygons fan-triangulated ``(0, i+1, i+2)``, texture images from ``map_Kd``
as float32 HWC in [0,1].  One-time setup work; stays on the host.
"""
import os
from collections import namedtuple

import numpy as np
import torch

Faces = namedtuple("Faces", "verts_idx normals_idx textures_idx materials_idx")
Properties = namedtuple("Properties", "normals verts_uvs material_colors texture_images texture_atlas")


def _parse_mtl(path):
    """-> (material_colors: {name: {...}}, texture_files: {name: filename})."""
    colors, tex = {}, {}
    cur = None
    if not os.path.isfile(path):
        return colors, tex
    with open(path, "r") as f:
        for line in f:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "newmtl":
                cur = tok[1]
                colors[cur] = {}
            elif cur is None:
                continue
            elif tok[0] == "map_Kd":
                tex[cur] = " ".join(tok[1:])
            elif tok[0] in ("Ka", "Kd", "Ks"):
                key = {"Ka": "ambient_color", "Kd": "diffuse_color", "Ks": "specular_color"}[tok[0]]
                colors[cur][key] = torch.tensor([float(t) for t in tok[1:4]], dtype=torch.float32)
            elif tok[0] == "Ns":
                colors[cur]["shininess"] = torch.tensor([float(tok[1])], dtype=torch.float32)
    return colors, tex


def _load_image_f32(path):
    from PIL import Image
    with Image.open(path) as im:
        arr = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(arr))


def load_obj(path, load_textures=True, device="cpu"):
    """Same return structure as ``pytorch3d.io.load_obj``: ``(verts, faces, aux)`` with
    ``faces.verts_idx`` / ``faces.textures_idx`` int64 (F,3) and ``aux.verts_uvs`` (VT,2),
    ``aux.texture_images`` {material: (H,W,3) float32}."""
    verts, uvs, normals = [], [], []
    f_v, f_t, f_n, f_m = [], [], [], []
    mtl_files, mat_names, cur_mat = [], [], -1
    with open(path, "r") as fh:
        for line in fh:
            if not line or line[0] == "#":
                continue
            tok = line.split()
            if not tok:
                continue
            k = tok[0]
            if k == "v":
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif k == "vt":
                uvs.append((float(tok[1]), float(tok[2])))
            elif k == "vn":
                normals.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif k == "mtllib":
                mtl_files.append(" ".join(tok[1:]))
            elif k == "usemtl":
                name = tok[1]
                if name not in mat_names:
                    mat_names.append(name)
                cur_mat = mat_names.index(name)
            elif k == "f":
                vi, ti, ni = [], [], []
                for t in tok[1:]:
                    parts = t.split("/")
                    a = int(parts[0])
                    vi.append(a - 1 if a > 0 else len(verts) + a)
                    if len(parts) > 1 and parts[1] != "":
                        b = int(parts[1])
                        ti.append(b - 1 if b > 0 else len(uvs) + b)
                    if len(parts) > 2 and parts[2] != "":
                        c = int(parts[2])
                        ni.append(c - 1 if c > 0 else len(normals) + c)
                for i in range(len(vi) - 2):            # fan triangulation
                    f_v.append((vi[0], vi[i + 1], vi[i + 2]))
                    f_t.append((ti[0], ti[i + 1], ti[i + 2]) if len(ti) == len(vi) else (-1, -1, -1))
                    f_n.append((ni[0], ni[i + 1], ni[i + 2]) if len(ni) == len(vi) else (-1, -1, -1))
                    f_m.append(cur_mat)

    def _t(lst, dtype, shape):
        if not lst:
            return torch.zeros(shape, dtype=dtype, device=device)
        return torch.tensor(lst, dtype=dtype, device=device)

    verts_t = _t(verts, torch.float32, (0, 3))
    has_uv = len(uvs) > 0 and all(t[0] >= 0 for t in f_t)
    faces = Faces(verts_idx=_t(f_v, torch.int64, (0, 3)),
                  normals_idx=_t(f_n, torch.int64, (0, 3)),
                  textures_idx=_t(f_t, torch.int64, (0, 3)) if has_uv else None,
                  materials_idx=_t(f_m, torch.int64, (0,)))
    colors, tex_images = {}, {}
    base = os.path.dirname(os.path.abspath(path))
    for m in mtl_files:
        c, tfiles = _parse_mtl(os.path.join(base, m))
        colors.update(c)
        if load_textures:
            for name, fn in tfiles.items():
                p = os.path.join(base, fn)
                if os.path.isfile(p):
                    tex_images[name] = _load_image_f32(p).to(device)
    aux = Properties(normals=_t(normals, torch.float32, (0, 3)) if normals else None,
                     verts_uvs=_t(uvs, torch.float32, (0, 2)) if uvs else None,
                     material_colors=colors or None,
                     texture_images=tex_images or None,
                     texture_atlas=None)
    return verts_t, faces, aux


def synthesize_uvs(verts):
    """UVs for meshes that ship without any (teapot, SURVEY.md D3 -- the reference would
    crash there, so there is no behaviour to match): spherical parametrisation about the
    centroid, per-vertex (faces_uvs == faces).  u = atan2(x,z)/(2pi)+0.5, v = acos(-y/r)/pi."""
    v = verts - verts.mean(dim=0, keepdim=True)
    r = v.norm(dim=1).clamp_min(1e-8)
    u = torch.atan2(v[:, 0], v[:, 2]) / (2 * torch.pi) + 0.5
    w = torch.acos((-v[:, 1] / r).clamp(-1, 1)) / torch.pi
    return torch.stack([u, w], dim=1).to(torch.float32)


def load_vertex_colors(path):
    """The per-vertex colours of an OBJ written with ``v x y z r g b`` lines (``save_obj(verts_colors=...)``, MeshLab's
    convention) -> (V,3) float32, or None when its ``v`` lines carry three numbers.  (``load_obj`` does not read them.)"""
    cols, plain = [], False
    with open(path, "r") as fh:
        for line in fh:
            tok = line.split("#", 1)[0].split()
            if not tok or tok[0] != "v":
                continue
            if len(tok) >= 7:
                cols.append((float(tok[4]), float(tok[5]), float(tok[6])))
            else:
                plain = True
    if plain or not cols:
        return None
    return torch.tensor(cols, dtype=torch.float32)


ATLAS_MAX_R = 64
ATLAS_SOUP_MAX_FACES = 2 ** 20      # the final export writes the triangle soup of an atlas up to this many sub-triangles


def _check_atlas_shape(shape, what):
    if len(shape) != 4 or shape[3] != 3 or shape[1] != shape[2] or not 1 <= shape[1] <= ATLAS_MAX_R or shape[0] < 1:
        raise ValueError(f"{what}: an atlas is (F, R, R, 3) with 1 <= R <= {ATLAS_MAX_R}, got {tuple(shape)}")


def save_atlas(path, atlas):
    """The (F,R,R,3) texels of a TexturesAtlas as a float32 ``.npy`` array."""
    _check_atlas_shape(tuple(atlas.shape), "save_atlas")
    with open(path, "wb") as fh:                # (np.save would append .npy to a path that lacks it)
        np.save(fh, atlas.detach().cpu().to(torch.float32).numpy())


def load_atlas(path):
    """``save_atlas``'s array -> (F,R,R,3) float32 tensor; ValueError when the file holds anything else."""
    arr = np.load(path, allow_pickle=False)
    _check_atlas_shape(arr.shape, f"load_atlas({path!r})")
    if arr.dtype.kind != "f":
        raise ValueError(f"load_atlas({path!r}): an atlas holds floats, got {arr.dtype}")
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))


def atlas_to_triangle_soup(verts, faces, atlas):
    """A mesh with a per-face texel atlas as the exact mesh it renders as: every face split into its R^2 sub-triangles, each
    with three vertices of its own that carry its texel's colour -> (verts' (3 F R^2, 3), faces' (F R^2, 3) int64, colours'
    (3 F R^2, 3)); sub-triangle (f R + y) R + x is texel atlas[f][y][x].  On the face's barycentric grid (b0, b1) = (i, j) / R:
    the lower sub-triangle of cell (i, j) has corners (i,j), (i+1,j), (i,j+1) and texel [j][i]; for i + j <= R - 2 the upper
    one has corners (i+1,j), (i+1,j+1), (i,j+1) and texel [R-1-j][R-1-i].  The winding is the parent's.  Pure torch, in the
    dtype of `verts`."""
    _check_atlas_shape(tuple(atlas.shape), "atlas_to_triangle_soup")
    faces = faces.reshape(-1, 3).to(torch.int64)
    verts = verts.reshape(-1, 3)
    n_faces, R = atlas.shape[0], atlas.shape[1]
    if faces.shape[0] != n_faces:
        raise ValueError(f"the atlas holds {n_faces} blocks for a mesh of {faces.shape[0]} faces")
    y, x = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    below = x + y < R
    i, j = torch.where(below, x, R - 1 - x), torch.where(below, y, R - 1 - y)
    # integer barycentric corners (a, b) of the three vertices of every texel's sub-triangle, (R,R,3)
    a = torch.stack([torch.where(below, i, i + 1), i + 1, i], dim=-1)
    b = torch.stack([j, torch.where(below, j, j + 1), j + 1], dim=-1)
    wa = a.reshape(-1).to(verts.dtype).to(verts.device)
    wb = b.reshape(-1).to(verts.dtype).to(verts.device)
    wc = R - wa - wb
    p = verts[faces]                                                                         # (F,3,3)
    pts = (wa[None, :, None] * p[:, 0, None, :] + wb[None, :, None] * p[:, 1, None, :] + wc[None, :, None] * p[:, 2, None, :]) / R
    soup_verts = pts.reshape(-1, 3)
    soup_faces = torch.arange(soup_verts.shape[0], dtype=torch.int64, device=verts.device).reshape(-1, 3)
    colours = atlas.reshape(-1, 1, 3).expand(-1, 3, 3).reshape(-1, 3)
    return soup_verts, soup_faces, colours


def save_obj(path, verts, faces, verts_uvs=None, faces_uvs=None, texture_map=None, decimal_places=6, verts_colors=None):
    """Writes ``<path>`` (+ ``.mtl`` + ``.png`` next to it when a texture is given), the
    artefact set of ``IO().save_mesh(final_mesh, .../final.obj)`` (first_approach.py:225).
    verts_colors (V,3): ``v x y z r g b`` lines with the colours clamped to [0,1] and the same decimal places."""
    from PIL import Image
    base, _ = os.path.splitext(path)
    stem = os.path.basename(base)
    verts = verts.detach().cpu().reshape(-1, 3).numpy()
    faces = faces.detach().cpu().reshape(-1, 3).numpy()
    with open(path, "w") as f:
        has_tex = texture_map is not None and verts_uvs is not None and faces_uvs is not None
        if has_tex:
            f.write(f"\nmtllib {stem}.mtl\nusemtl mesh\n\n")
        fmt = f"%.{decimal_places}f"
        if verts_colors is not None:
            cols = verts_colors.detach().cpu().reshape(-1, 3).clamp(0, 1).numpy()
            if cols.shape[0] != verts.shape[0]:
                raise ValueError(f"verts_colors holds {cols.shape[0]} colours for {verts.shape[0]} vertices")
            verts = np.concatenate([verts, cols], axis=1)
        for v in verts:
            f.write("v " + " ".join(fmt % x for x in v) + "\n")
        if has_tex:
            uv = verts_uvs.detach().cpu().reshape(-1, 2).numpy()
            fuv = faces_uvs.detach().cpu().reshape(-1, 3).numpy()
            for t in uv:
                f.write("vt " + " ".join(fmt % x for x in t) + "\n")
            for a, b in zip(faces, fuv):
                f.write("f " + " ".join(f"{int(i) + 1}/{int(j) + 1}" for i, j in zip(a, b)) + "\n")
        else:
            for a in faces:
                f.write("f " + " ".join(str(int(i) + 1) for i in a) + "\n")
    if has_tex:
        tex = texture_map.detach().cpu().reshape(texture_map.shape[-3], texture_map.shape[-2], 3)
        img = (tex.clamp(0, 1) * 255.0).round().to(torch.uint8).numpy()
        Image.fromarray(img).save(base + ".png")
        with open(base + ".mtl", "w") as f:
            f.write(f"newmtl mesh\nmap_Kd {stem}.png\nKa 1.000 1.000 1.000\nKd 1.000 1.000 1.000\n"
                    "Ks 0.000 0.000 0.000\nNs 10.0\n")
