"""Every wrapper of st3d/bake.py between guard zones (tests/_guarded.py): no write outside its outputs, no read of memory it did
not write, and the same bits under both fill patterns and in a plain run."""
import numpy as np
import pytest
import torch

import _bakeref as BR
import _guarded as G
import _scenes

pytestmark = pytest.mark.gpu
MODULES = ("st3d.bake",)
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_every_wrapper_between_guard_zones(dev):
    import utils as U
    from st3d import bake, ops
    from st3d.render import FoVPerspectiveCameras
    U.device = dev
    S, T = 33, 31                                    # odd sides: the last workgroup of every launch is partly idle
    cow = _scenes.load_asset("cow")
    verts, faces = _t(cow["verts"], dev), _t(cow["faces"].astype(np.int32), dev)
    uvs, fuv = _t(cow["verts_uvs"].astype(np.float32), dev), _t(cow["faces_uvs"].astype(np.int32), dev)
    R, Tr = _scenes.random_cameras(5, 0)
    dR, dT = _t(R, dev), _t(Tr, dev)
    want_f, want_b, unsure = BR.surface(cow["verts_uvs"], cow["faces_uvs"], T, 1.5)

    out = G.compare_ab(lambda: dict(zip(("t2f", "tbary"), bake.texel_surface(uvs, fuv, T))), modules=MODULES)
    t2f, tbary = out["t2f"].clone(), out["tbary"].clone()
    ok = ~unsure
    assert np.array_equal(t2f.cpu().numpy()[ok], want_f[ok]) and (want_f >= 0).sum() > 100
    out = G.compare_ab(lambda: dict(zip(("t2f", "tbary"), bake.texel_surface(uvs, fuv, T, 0.0))), modules=MODULES)
    assert int((out["t2f"] >= 0).sum()) < int((t2f >= 0).sum())

    p2f, zbuf, _, _ = ops.raster_fwd(ops.project_verts(verts, dR, dT), faces, S)
    imgs = _t(np.random.default_rng(3).random((5, 3, S, S)).astype(np.float32), dev)
    for mode in ("mean", "best"):
        fresh = G.compare_ab(lambda: {"acc": bake.bake_views(verts, faces, t2f, tbary, dR, dT, imgs, p2f, zbuf, mode=mode)},
                             modules=MODULES)
        assert int((fresh["acc"][..., 3] > 0).sum()) > 50 and bool((fresh["acc"][t2f < 0] == 0).all())
        head = bake.bake_views(verts, faces, t2f, tbary, dR[:2].contiguous(), dT[:2].contiguous(), imgs[:2].contiguous(),
                               p2f[:2].contiguous(), zbuf[:2].contiguous(), mode=mode)

        def into_own():
            mine = head.clone()
            return {"acc": bake.bake_views(verts, faces, t2f, tbary, dR[2:].contiguous(), dT[2:].contiguous(), imgs[2:].contiguous(),
                                           p2f[2:].contiguous(), zbuf[2:].contiguous(), mode=mode, acc=mine)}
        cont = G.compare_ab(into_own, modules=MODULES, own=lambda o: [o["acc"]])
        assert torch.equal(cont["acc"].view(I32), fresh["acc"].view(I32))

    acc = fresh["acc"].clone()
    fallback = _t(np.random.default_rng(4).random((T, T, 3)).astype(np.float32), dev)
    out = G.compare_ab(lambda: {"texture": bake.baked_texture(acc, fallback)}, modules=MODULES)
    unwritten = acc[..., 3] == 0
    assert torch.equal(out["texture"][unwritten], fallback[unwritten]) and int((~unwritten).sum()) > 50

    mesh = U.build_mesh(uvs[None], _t(cow["faces_uvs"].astype(np.int64), dev)[None], fallback[None].clone(), verts,
                        _t(cow["faces"].astype(np.int64), dev))
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(Tr), device=dev)

    def whole():
        texture, total = bake.bake_texture(mesh, imgs, cams, S, mode="best", batch=2)       # 2 + 2 + 1 views
        return {"texture": texture, "acc": total}
    out = G.compare_ab(whole, modules=MODULES)
    assert torch.equal(out["acc"].view(I32), acc.view(I32))             # batched = one launch over all views, bit for bit
    assert torch.equal(out["texture"].view(I32), bake.baked_texture(acc, fallback).view(I32))
