"""csrc/cover.hip and st3d/cover.py on the GPU against tests/_coverref.py, bit for bit: the marks on the GPU's own fragments,
the greedy rounds on random masks with planted duplicates and empty rows, the counts, select_cameras end to end, every
wrapper between guard zones, and one short second_approach run with and without the flags."""
import os
import re

import numpy as np
import pytest
import torch

import _coverref as CR
import _guarded as G
import _scenes

pytestmark = pytest.mark.gpu
MODULES = ("st3d.cover",)
I32 = torch.int32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cover():
    from st3d import cover
    return cover


class _Scene:
    """the cow on the device, and the GPU's own hard fragments per (views, side), rasterised and downloaded once"""

    def __init__(self, dev):
        self.dev = dev
        self.cow = _scenes.load_asset("cow")
        self.verts = torch.from_numpy(self.cow["verts"]).to(dev)
        self.faces = torch.from_numpy(self.cow["faces"].astype(np.int32)).to(dev)
        self.uvs = torch.from_numpy(self.cow["verts_uvs"].astype(np.float32)).to(dev)
        self.fuv = torch.from_numpy(self.cow["faces_uvs"].astype(np.int32)).to(dev)
        self._frags = {}

    def frags(self, C, S):
        """-> (device fragments of ops.raster_fwd, the same per view as numpy tuples)"""
        if (C, S) not in self._frags:
            from st3d import ops
            R, T = _scenes.random_cameras(C, 0)
            ndc = ops.project_verts(self.verts, torch.from_numpy(R).to(self.dev), torch.from_numpy(T).to(self.dev))
            frag = ops.raster_fwd(ndc, self.faces, S)
            host = [t.cpu().numpy() for t in frag]
            self._frags[(C, S)] = (frag, [tuple(h[b] for h in host) for b in range(C)])
        return self._frags[(C, S)]

    def reference(self, C, S, T):
        return CR.mark(self.frags(C, S)[1], self.cow["verts_uvs"], self.cow["faces_uvs"], T)

    def mesh(self, T):
        import utils as U
        tex = torch.from_numpy(_scenes.texture_at(self.cow, T))[None].to(self.dev)
        return U.build_mesh(self.uvs[None], torch.from_numpy(self.cow["faces_uvs"].astype(np.int64))[None].to(self.dev), tex,
                            self.verts, torch.from_numpy(self.cow["faces"].astype(np.int64)).to(self.dev))


@pytest.fixture(scope="module")
def scene(dev):
    return _Scene(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------- 1. mark
@pytest.mark.parametrize("T", [8, 31, 32, 33, 64])
@pytest.mark.parametrize("S", [16, 17, 33])
def test_marks_equal_the_restatement_on_the_gpus_own_fragments(cover, scene, dev, S, T):
    frag, _ = scene.frags(3, S)
    want = scene.reference(3, S, T)
    assert CR.popcount(want) > 0
    got = cover.mark_texels(frag, scene.uvs, scene.fuv, T)
    assert got.dtype == I32 and tuple(got.shape) == (3, cover.words(T))
    assert np.array_equal(_np(got), want)
    if T * T % 32:
        assert not (CR.as_u32(_np(got))[:, -1] >> np.uint32(T * T % 32)).any()         # tail bits are zero
    assert torch.equal(cover.unpack(got, T), _t(CR.unpack(want, T), dev))
    again = cover.mark_texels(frag, scene.uvs, scene.fuv, T)
    assert torch.equal(again, got)                                                       # two runs, the same bits
    rng = np.random.default_rng(S * 100 + T)
    before = rng.integers(-2 ** 31, 2 ** 31, size=want.shape, dtype=np.int64).astype(np.int32)
    filled = _t(before, dev)
    out = cover.mark_texels(frag, scene.uvs, scene.fuv, T, masks=filled)
    assert out is filled and np.array_equal(CR.as_u32(_np(out)), CR.as_u32(before) | CR.as_u32(want))   # earlier bits stay


# ---------------------------------------------------------------------------- 2. greedy
def _random_masks(rng, C, W):
    """rows of very different densities, a duplicate of row 0, an all-zero row and a copy of the densest row (when C allows)"""
    density = rng.uniform(0.01, 0.6, size=(C, 1))
    bits = rng.random((C, W, 32)) < density[:, :, None]
    m = (bits.astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)
    if C >= 3:
        m[C // 2] = m[0]
        m[C - 1] = 0
    if C >= 5:
        m[1] = m[np.argmax(density[:, 0])]
    return CR.as_i32(m)


@pytest.mark.parametrize("C", [1, 5, 70, 257])
def test_greedy_equals_numpy_on_random_masks(cover, dev, C):
    rng = np.random.default_rng(C)
    for W in (1, 2, 33, 257, 36, 64):               # 36 and 64: rows read 16 bytes at a time
        masks = _random_masks(rng, C, W)
        start = CR.as_i32(((rng.random((W, 32)) < 0.1).astype(np.uint32) << np.arange(32, dtype=np.uint32))
                          .sum(-1, dtype=np.uint32))
        dm, ds = _t(masks, dev), _t(start, dev)
        for n in sorted({1, max(1, C // 2), C}):
            for covered, dcov in ((None, None), (start, ds)):
                wp, wg, wc = CR.greedy(masks, n, covered)
                picks, gains, cov = cover.greedy_views(dm, n, dcov)
                assert picks.dtype == I32 and gains.dtype == I32 and cov.dtype == I32
                assert np.array_equal(_np(picks), wp), (C, W, n)
                assert np.array_equal(_np(gains), wg), (C, W, n)
                assert np.array_equal(_np(cov), wc), (C, W, n)
                assert len(set(wp.tolist())) == n
        assert np.array_equal(_np(ds), start) and np.array_equal(_np(dm), masks)          # the inputs are not written


def test_greedy_goes_on_in_index_order_once_nothing_is_left_to_gain(cover, dev):
    masks = CR.as_i32(np.array([[0xFFFFFFFF, 0xF], [0xFFFFFFFF, 0xF], [0, 0], [0xFFFFFFFF, 0xF]], np.uint32))
    picks, gains, cov = cover.greedy_views(_t(masks, dev), 4)
    assert _np(picks).tolist() == [0, 1, 2, 3] and _np(gains).tolist() == [36, 0, 0, 0] and CR.popcount(_np(cov)) == 36
    tie = CR.as_i32(np.array([[1, 0], [0, 0b111], [0b111, 0]], np.uint32))
    assert _np(cover.greedy_views(_t(tie, dev), 2)[0]).tolist() == [1, 2]               # ties go to the lowest index


# ---------------------------------------------------------------------------- 3. count
@pytest.mark.parametrize("T", [5, 31, 32, 64])
def test_counts_equal_the_sum_of_the_unpacked_masks(cover, dev, T):
    rng = np.random.default_rng(T)
    touch = rng.random((7, T, T)) < rng.uniform(0.05, 0.9, size=(7, 1, 1))
    masks = _t(CR.pack(touch), dev)
    counts = cover.coverage_counts(masks, T)
    assert counts.dtype == I32 and tuple(counts.shape) == (T, T)
    assert torch.equal(counts, cover.unpack(masks, T).sum(0).to(I32))
    assert np.array_equal(_np(counts), touch.sum(0)) and np.array_equal(_np(counts), CR.count(_np(masks), T))


# ---------------------------------------------------------------------------- 4. end to end
def test_select_cameras_picks_what_the_restatement_picks(cover, scene, dev):
    from st3d.render import FoVPerspectiveCameras
    C, S, T, n = 24, 32, 32, 6
    R, Tr = _scenes.random_cameras(C, 0)
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(Tr), device=dev)
    mesh = scene.mesh(T)
    masks = cover.texel_masks(mesh, cams.R, cams.T, S)
    want_masks = scene.reference(C, S, T)
    assert np.array_equal(_np(masks), want_masks)           # rasterised eight views at a time: the same fragments
    assert np.array_equal(_np(cover.texel_masks(mesh, cams.R, cams.T, S, batch=5)), want_masks)
    wp, wg, wc = CR.greedy(want_masks, n)
    chosen, report = cover.select_cameras(mesh, cams, n, S)
    print("report", {k: v for k, v in report.items() if k != "counts"})
    assert report["picks"] == wp.tolist() and report["gains"] == wg.tolist() and report["candidates"] == C
    assert report["pool"] == CR.reached(want_masks) and report["picked"] == CR.popcount(wc) == sum(report["gains"])
    assert report["first_n"] == CR.reached(want_masks[:n])
    assert report["picked"] > report["first_n"] and report["pool"] >= report["picked"]
    assert np.array_equal(_np(report["counts"]), CR.count(want_masks[wp], T))
    assert len(chosen) == n and np.array_equal(_np(chosen.R), R[wp]) and np.array_equal(_np(chosen.T), Tr[wp])
    import utils as U
    U.device = dev
    gen = torch.Generator().manual_seed(0)
    a, ra = U.build_coverage_cameras(4, mesh, S, candidates=16, generator=gen)
    b, rb = U.build_coverage_cameras(4, mesh, S, candidates=16, generator=torch.Generator().manual_seed(0))
    assert ra["picks"] == rb["picks"] and torch.equal(a.R, b.R) and torch.equal(a.T, b.T)       # a pure function of the seed
    pool = U.build_random_cameras(16, generator=torch.Generator().manual_seed(0))
    assert torch.equal(a.R, pool.R[torch.tensor(ra["picks"], device=pool.R.device)])


# ---------------------------------------------------------------------------- 5. between guard zones
def test_every_wrapper_between_guard_zones(cover, scene, dev):
    from st3d.render import FoVPerspectiveCameras
    S, T = 17, 33
    frag, _ = scene.frags(3, S)
    want = scene.reference(3, S, T)
    out = G.compare_ab(lambda: {"masks": cover.mark_texels(frag, scene.uvs, scene.fuv, T)}, modules=MODULES)
    assert np.array_equal(_np(out["masks"]), want)
    before = _t(CR.pack(np.random.default_rng(1).random((3, T, T)) < 0.2), dev)

    def into_own():
        mine = before.clone()
        return {"masks": cover.mark_texels(frag, scene.uvs, scene.fuv, T, masks=mine)}
    out = G.compare_ab(into_own, modules=MODULES, own=lambda o: [o["masks"]])
    assert np.array_equal(CR.as_u32(_np(out["masks"])), CR.as_u32(_np(before)) | CR.as_u32(want))
    rng = np.random.default_rng(2)
    for C, W, n in ((70, 33, 35), (70, 36, 70)):
        masks = _random_masks(rng, C, W)
        dm = _t(masks, dev)
        start = _t(masks[3], dev)

        def greedy():
            picks, gains, cov = cover.greedy_views(dm, n, start)
            return {"picks": picks, "gains": gains, "covered": cov}
        out = G.compare_ab(greedy, modules=MODULES)
        wp, wg, wc = CR.greedy(masks, n, masks[3])
        assert np.array_equal(_np(out["picks"]), wp) and np.array_equal(_np(out["gains"]), wg)
        assert np.array_equal(_np(out["covered"]), wc)
    dw = _t(want, dev)
    out = G.compare_ab(lambda: {"counts": cover.coverage_counts(dw, T)}, modules=MODULES)
    assert np.array_equal(_np(out["counts"]), CR.count(want, T))
    R, Tr = _scenes.random_cameras(12, 0)
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(Tr), device=dev)
    mesh = scene.mesh(T)
    ref12 = scene.reference(12, S, T)
    out = G.compare_ab(lambda: {"masks": cover.texel_masks(mesh, cams.R, cams.T, S, batch=5)}, modules=MODULES)
    assert np.array_equal(_np(out["masks"]), ref12)

    def select():
        chosen, report = cover.select_cameras(mesh, cams, 4, S)
        return {"counts": report["counts"], "_picks": report["picks"]}
    out = G.compare_ab(select, modules=MODULES)
    assert np.array_equal(_np(out["counts"]), CR.count(ref12[CR.greedy(ref12, 4)[0]], T))


# ---------------------------------------------------------------------------- 6. the CLI
def _write_cow_assets(tmp, cow, golden_dir, tex_size=64):
    from PIL import Image
    from st3d import io as stio
    tex = torch.from_numpy(cow["texture_u8"][::1024 // tex_size, ::1024 // tex_size].copy()).float() / 255
    obj = os.path.join(tmp, "cow.obj")
    stio.save_obj(obj, torch.from_numpy(cow["verts"]), torch.from_numpy(cow["faces"].astype(np.int64)),
                  torch.from_numpy(cow["verts_uvs"]), torch.from_numpy(cow["faces_uvs"].astype(np.int64)), tex)
    style = os.path.join(tmp, "style.png")
    Image.fromarray(np.load(os.path.join(golden_dir, "assets_style1_512.npz"))["rgb_u8"]).save(style)
    return obj, style


def test_second_approach_with_coverage_and_unchanged_without(dev, cow, golden_dir, tmp_path, capsys):
    import losses as L
    import second_approach as SA
    import style_transfer as ST
    import utils as U
    from PIL import Image
    U.device = ST.device = L.device = dev
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "32", "--n_views", "4", "--batch_size", "4", "--epochs", "2",
              "--seed", "0", "--save_every", "0"]
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    capsys.readouterr()
    SA.main(common + ["--view_selection", "coverage", "--view_candidates", "16", "--output_path", on])
    said = capsys.readouterr().out
    line = re.search(r"View selection: the 4 picked of 16 candidates reach (\d+) of the (\d+) texels the candidates reach together; "
                     r"the first 4 candidates reach (\d+)", said)
    assert line, said
    picked, pool, first = (int(v) for v in line.groups())
    print("coverage line", picked, pool, first)
    assert 0 < first <= picked <= pool <= 32 * 32
    png = Image.open(os.path.join(on, "texel_coverage.png"))
    assert png.size == (32, 32)
    shade = np.asarray(png.convert("L"))
    assert (shade > 0).sum() == picked and shade.max() <= 255
    losses = [float(l.split("Loss ")[1]) for l in open(os.path.join(on, "log.txt")).read().splitlines()[1:]]
    assert len(losses) == 2 and all(np.isfinite(losses))
    SA.main(common + ["--output_path", off])
    assert "View selection" not in capsys.readouterr().out and not os.path.exists(os.path.join(off, "texel_coverage.png"))
    # the log of this command as the commit before this feature writes it (recorded on an MI355X)
    want = open(os.path.join(golden_dir, "cover_cli_parent_log.txt"), "rb").read()
    assert open(os.path.join(off, "log.txt"), "rb").read() == want
