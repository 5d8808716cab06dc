"""fp64 torch restatement of PyTorch3D's Phong lighting (SoftPhongShader -> phong_shading, PointLights / DirectionalLights
.diffuse / .specular, Meshes.verts_normals_packed), written from the formulas, for the lighting tests.  It composes with
oracle/soft_ref.py: sample_texture gives the texels, these functions light them, softmax_rgb_blend blends.

World space throughout; X_view = X_world R + T, so the camera centre is C = -T R^T.

  verts_normals_packed:  c_f = (v2 - v1) x (v0 - v1) per face (area-weighted, unnormalised), m_v = sum of c_f over the
                         faces of v, n_v = m_v / max(|m_v|, 1e-6)
  per fragment:          N = sum_i b_i n_{f,i} (not renormalised), P = sum_i b_i v_{f,i}
  light direction:       L = location - P (PointLights) | direction (DirectionalLights, pointing towards the light);
                         normalize(x) = x / max(|x|, 1e-6); n = normalize(N), l = normalize(L)
  diffuse:               D = kd Ld relu(n.l)
  specular:              cos = n.l, r = -l + 2 cos n, e = normalize(C - P), alpha = relu(e.r) [cos > 0],
                         Sp = ks Ls alpha^shininess
  ambient:               A = ka La
  colour:                (A + D) texel + Sp -- no clamping; it replaces the texel in softmax_rgb_blend; the background is
                         not lit.
"""
import torch

EPS = 1e-6


def normalize(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)


def vertex_normals(verts, faces):
    """verts (V,3), faces (F,3) long -> (V,3) unit vertex normals (Meshes.verts_normals_packed)."""
    v0, v1, v2 = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    c = torch.cross(v2 - v1, v0 - v1, dim=1)
    m = torch.zeros_like(verts)
    for i in range(3):
        m = m.index_add(0, faces[:, i], c)
    return normalize(m)


def camera_centre(R, T):
    """R (3,3), T (3,) -> C = -T R^T"""
    return -(R @ T)


def interpolate(bary, p2f, faces, values):
    """sum_i b_i values[faces[f, i]] per fragment: bary (...,3), p2f (...) long -> (...,3)"""
    f = p2f.clamp_min(0)
    return sum(bary[..., i:i + 1] * values[faces[f, i]] for i in range(3))


def phong(N, P, C, light, material):
    """-> (A + D, Sp) per fragment, both (...,3).  light: dict(kind 'ambient' | 'point' | 'directional', ambient, diffuse,
    specular, location | direction), material: dict(ambient, diffuse, specular, shininess); colours (3,) tensors."""
    A = material["ambient"] * light["ambient"]
    if light["kind"] == "ambient":
        return A.expand(N.shape), torch.zeros_like(N)
    L = light["location"] - P if light["kind"] == "point" else light["direction"].expand(P.shape)
    n, l = normalize(N), normalize(L)
    cos = (n * l).sum(-1, keepdim=True)
    D = material["diffuse"] * light["diffuse"] * torch.relu(cos)
    r = -l + 2.0 * cos * n
    e = normalize(C - P)
    alpha = torch.relu((e * r).sum(-1, keepdim=True)) * (cos > 0).to(N.dtype)
    Sp = material["specular"] * light["specular"] * torch.pow(alpha, material["shininess"])
    return A + D, Sp


def lit_colors(texels, bary, p2f, verts, normals, faces, C, light, material):
    """texels (S,S,K,3) -> lit colours (A + D) texel + Sp (S,S,K,3)"""
    N = interpolate(bary, p2f, faces, normals)
    P = interpolate(bary, p2f, faces, verts)
    ad, sp = phong(N, P, C, light, material)
    return ad * texels + sp


def kink_margin(bary, p2f, verts, normals, faces, C, light):
    """per fragment: min(|n.l|, |e.r|) -- distance to the relu / [cos > 0] kinks where fp32 and fp64 can disagree"""
    N = interpolate(bary, p2f, faces, normals)
    P = interpolate(bary, p2f, faces, verts)
    if light["kind"] == "ambient":
        return torch.full(N.shape[:-1], float("inf"), dtype=N.dtype)
    L = light["location"] - P if light["kind"] == "point" else light["direction"].expand(P.shape)
    n, l = normalize(N), normalize(L)
    cos = (n * l).sum(-1)
    r = -l + 2.0 * cos[..., None] * n
    er = (normalize(C - P) * r).sum(-1)
    return torch.minimum(cos.abs(), er.abs())
