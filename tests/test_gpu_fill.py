"""--fill_unseen on the GPU: st3d_fill_pushpull (csrc/fill.hip) against its restatement (tests/_fillref.py), and the flag end
to end on all three scripts.

Tolerance of a filled texel against the fp64 restatement, counted from the roundings written in fill.hip (built with
-ffp-contract=off and the correctly rounded division, so they are the ones that happen).  u = 2^-24, M = max |valid colour|,
n = ceil(log2 max(H, W)) = the number of levels above the map.
  * Every weight is exactly 0 or 1 (level 0 is a select; a sum of such weights cut at 1 is 0 or 1 again), so the products
    w c of the pull are exact, W is a small integer, exact, and every "W > 0" / "w >= 1" decision is the restatement's.
  * pull_texel, per channel: up to three additions and one division round, a convex combination of the children: its own
    error is at most 4 u M (1 + O(u)), and it passes its children's errors on without growing them.  Level l carries at
    most 4 l u M.
  * push_texel, per channel: the tap weights and their products (sixteenths) are exact; four products (wy wx) c and three
    additions round, of which a first-order count is again 4 u M; with w = 0 the mix w c + (1 - w) up = 0 + 1 up is exact.
    A convex combination of the completed coarser level: a completed level l carries at most 4 n u M (its deepest pull)
    + 4 (n - l) u M (the pushes above it).
  * Level 0: 8 n u M.  One more u M covers the second-order terms ((1 + u)^(8 n) - 1 - 8 n u < u for n <= 14) and the
    rounding of the restatement's fp64 result to compare.
  bound = (8 n + 1) 2^-24 M.  (The issue's count of 17 per level assumed fractional weights, which this contract cannot
  produce.)  The restatement run in fp32 (same operations, same order) is the source rounding for rounding: the filled
  texels are also compared with it bit for bit.
"""
import os
import re

import numpy as np
import pytest
import torch

import _fillref as FR

pytestmark = pytest.mark.gpu
U_ = 2.0 ** -24
TAIL_SIDE = 64                  # fill.hip's kTailSide: the tail takes level 1 iff max(H, W) <= 128
SHAPES = [(1, 1), (1, 2), (2, 2), (3, 5), (8, 8), (33, 17), (2 * TAIL_SIDE - 1, 40), (2 * TAIL_SIDE, 2 * TAIL_SIDE),
          (2 * TAIL_SIDE + 1, 2 * TAIL_SIDE + 1), (130, 70), (300, 5)]       # (300, 5): two plain pull launches before the tail
MASKS = ("2%", "50%", "98%", "all", "none", "corner")
_REF = {}                       # (H, W, mask) -> the inputs and both restatements, computed once


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fill():
    from st3d import fill
    return fill


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # a copy: the shared references are read-only


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _mask(H, W, kind, rng):
    if kind.endswith("%"):
        return (rng.random((H, W)) < float(kind[:-1]) / 100).astype(np.uint8)
    valid = np.full((H, W), 1 if kind == "all" else 0, np.uint8)
    if kind == "corner":
        valid[H - 1, 0] = 1
    if kind == "hole":
        valid[:] = 1
        valid[45:85, 15:55] = 0
    return valid


def _case(H, W, kind):
    key = (H, W, kind)
    if key not in _REF:
        rng = np.random.default_rng([H, W, MASKS.index(kind) if kind in MASKS else 99])
        tex = rng.random((H, W, 3), dtype=np.float32)
        valid = _mask(H, W, kind, rng)
        out64, n, d64 = FR.push_pull(tex, valid)
        out32, _, _ = FR.push_pull(tex, valid, dtype=np.float32)
        for a in (tex, valid, out64, out32, d64["filled"], d64["take"]):
            a.setflags(write=False)
        _REF[key] = dict(tex=tex, valid=valid, out32=out32, count=n, filled=d64["filled"], take=d64["take"])
    return _REF[key]


def _check_case(fill, dev, monkeypatch, H, W, kind):
    """every check of the issue on one (shape, mask) -> the largest error as a share of the bound (0 when nothing is filled)"""
    c = _case(H, W, kind)
    tex, valid, take = c["tex"], c["valid"], c["take"]
    d_tex, d_valid = _t(tex, dev), _t(valid, dev)
    out, count = fill.push_pull(d_tex, d_valid)
    got = out.cpu().numpy()
    label = f"{H}x{W} {kind}"
    assert int(count) == c["count"] == int(take.sum()), label
    assert np.array_equal(got.view(np.uint32)[~take], tex.view(np.uint32)[~take]), label      # valid texels: bit for bit
    assert np.array_equal(got.view(np.uint32), c["out32"].view(np.uint32)), label             # the fp32 restatement's bits
    share = 0.0
    if take.any():
        n = len(FR.level_sides(H, W)) - 1
        assert n == int(np.ceil(np.log2(max(H, W))))
        bound = (8 * n + 1) * U_ * float(np.abs(tex[valid != 0]).max())
        err = float(np.abs(got.astype(np.float64) - c["filled"])[take].max())
        share = err / bound
        assert err <= bound, (label, err, bound)
    again, count2 = fill.push_pull(d_tex, d_valid)
    assert np.array_equal(_bits(again), got.view(np.uint32)) and int(count2) == c["count"], label     # two runs
    with monkeypatch.context() as m:
        m.setenv("ST3D_FILL_TAIL", "0")
        plain, count3 = fill.push_pull(d_tex, d_valid)
        torch.cuda.synchronize()
    assert np.array_equal(_bits(plain), got.view(np.uint32)) and int(count3) == c["count"], label     # every level a launch
    for junk in (np.nan, 3e38):                             # what invalid texels hold reaches nothing
        dirty = tex.copy()
        dirty[valid == 0] = junk
        soiled, count4 = fill.push_pull(_t(dirty, dev), d_valid)
        assert np.array_equal(_bits(soiled)[take], got.view(np.uint32)[take]) and int(count4) == c["count"], (label, junk)
        assert np.array_equal(_bits(soiled)[~take], dirty.view(np.uint32)[~take]), (label, junk)
    flat = np.full((H, W, 3), 0.3, np.float32) * np.array([1.0, 2.0, 3.0], np.float32)
    const, _ = fill.push_pull(_t(flat, dev), d_valid)
    ulps = np.abs(_bits(const).astype(np.int64) - flat.view(np.uint32).astype(np.int64))
    assert ulps.max() <= 4, (label, int(ulps.max()))
    return share


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_matches_its_restatement(fill, dev, monkeypatch, shape):
    H, W = shape
    shares = {kind: _check_case(fill, dev, monkeypatch, H, W, kind) for kind in MASKS}
    print(f"fill {H}x{W}: largest error / bound per mask", {k: round(v, 4) for k, v in shares.items()})


def test_a_40x40_hole_is_filled_from_the_coarse_levels(fill, dev, monkeypatch):
    share = _check_case(fill, dev, monkeypatch, 130, 70, "hole")
    c = _case(130, 70, "hole")
    assert c["count"] == 1600
    lo, hi = c["tex"][c["valid"] != 0].min(), c["tex"][c["valid"] != 0].max()
    out, _ = fill.push_pull(_t(c["tex"], dev), _t(c["valid"], dev))
    inner = out.cpu().numpy()[55:75, 25:45]                 # ten texels from the rim: only levels 3 and coarser reach here
    assert lo <= inner.min() and inner.max() <= hi and inner.std() < 0.25 * c["tex"].std()
    print(f"fill 130x70 hole: error / bound {share:.4f}")


def test_domain_limits_the_writes_but_not_the_sources(fill, dev, monkeypatch):
    for (H, W), kind in (((130, 70), "50%"), ((33, 17), "2%"), ((300, 5), "98%")):
        c = _case(H, W, kind)
        tex, valid = c["tex"], c["valid"]
        domain = (np.random.default_rng(7).random((H, W)) < 0.5).astype(np.uint8)
        want, n, _ = FR.push_pull(tex, valid, domain, dtype=np.float32)
        whole, _ = fill.push_pull(_t(tex, dev), _t(valid, dev))
        for tail in ("1", "0"):
            with monkeypatch.context() as m:
                m.setenv("ST3D_FILL_TAIL", tail)
                out, count = fill.push_pull(_t(tex, dev), _t(valid, dev), _t(domain, dev))
                torch.cuda.synchronize()
            got = _bits(out)
            inside = domain != 0
            assert int(count) == n == int(((valid == 0) & inside).sum()) > 0
            assert np.array_equal(got[~inside], tex.view(np.uint32)[~inside])          # outside the domain: the input's bits
            assert np.array_equal(got[inside], _bits(whole)[inside])                   # inside: the undomained fill's colours
            assert np.array_equal(got, want.view(np.uint32))


def test_wrappers_refuse_what_the_library_would_misread(fill, dev):
    from st3d._lib import St3dError
    ok = torch.ones(8, 6, dtype=torch.uint8, device=dev)
    with pytest.raises(St3dError, match="contiguous"):
        fill.push_pull(torch.zeros(6, 8, 3, device=dev).transpose(0, 1), ok)
    with pytest.raises(St3dError, match="contiguous"):
        fill.push_pull(torch.zeros(8, 6, 3, device=dev), torch.ones(6, 8, dtype=torch.uint8, device=dev).t())
    with pytest.raises(St3dError, match="CPU tensor"):
        fill.push_pull(torch.zeros(8, 6, 3, device=dev), ok.cpu())
    tex = torch.rand(8, 6, 3, device=dev)
    original = tex.clone()
    tex[2, 3] = torch.tensor([1.5, 2.25, 3.0], device=dev)         # a few bits each: every product of the push is exact
    filled, count = fill.fill_unseen(tex, original)
    assert int(count) == 47 and torch.equal(filled, tex[2, 3].expand(8, 6, 3))      # the one moved texel colours the map


# ---------------------------------------------------------------------------- the scripts
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


def _final_map(folder):
    from st3d import io as stio
    _, _, aux = stio.load_obj(os.path.join(folder, "final.obj"))
    t = next(iter(aux.texture_images.values()))
    return (t.detach().cpu().clamp(0, 1) * 255.0).round().to(torch.uint8).numpy()


_STEPS = {"first_approach": ["--n_style_transfer_steps", "2", "--n_mse_steps", "3"],
          "second_approach": ["--epochs", "3", "--save_every", "0"],
          "third_approach": ["--n_rounds", "1", "--n_style_transfer_steps", "2", "--n_mse_steps", "3"]}


@pytest.mark.parametrize("script", sorted(_STEPS))
def test_script_fills_at_export_and_is_unchanged_with_the_flag_off(script, fill, dev, cow, golden_dir, tmp_path, capsys, monkeypatch):
    import importlib
    import losses as L
    import style_transfer as ST
    import utils as U
    from PIL import Image
    from st3d import bake, cli
    U.device = ST.device = L.device = dev
    mod = importlib.import_module(script)
    obj, style = _write_cow_assets(str(tmp_path), cow, golden_dir)
    common = ["--obj_path", obj, "--style_path", style, "--size", "64", "--n_views", "2", "--batch_size", "2", "--seed", "0"] \
        + _STEPS[script]
    seen = {}
    real_export = cli.Run.export

    def export(self, mesh):                                 # what the run hands over, and what it started from
        seen["leaf"] = mesh.textures.maps_padded().detach().clone()[0]
        seen["original"] = self.original_map.detach().clone()[0]
        seen["uvs"] = mesh.textures.verts_uvs_padded().detach().reshape(-1, 2).float().contiguous()
        seen["fuv"] = mesh.textures.faces_uvs_i32()
        return real_export(self, mesh)
    monkeypatch.setattr(cli.Run, "export", export)
    monkeypatch.setattr(U.random, "shuffle", lambda plan: None)         # the turntable in the same order in every run
    folders = {k: str(tmp_path / k) for k in ("plain", "off", "chart", "map")}
    said = {}
    capsys.readouterr()
    for k, folder in folders.items():
        mod.main(common + ([] if k == "plain" else ["--fill_unseen", k]) + ["--output_path", folder])
        said[k] = capsys.readouterr().out
    log = lambda k: open(os.path.join(folders[k], "log.txt"), "rb").read()
    final = {k: _final_map(folders[k]) for k in folders}
    # off = no flag: the same log, the same map, no line, no picture
    assert log("off") == log("plain") and len(log("off").splitlines()) >= 2
    assert np.array_equal(final["off"], final["plain"])
    for k in ("off", "plain"):
        assert "Fill:" not in said[k] and not os.path.exists(os.path.join(folders[k], "texel_filled.png"))
    # the texels of the off run (every run hands over the same leaf: the logs agree and the fill comes after the last step)
    moved = fill.moved_texels(seen["leaf"].contiguous(), seen["original"].contiguous()).cpu().numpy() != 0
    chart = (bake.texel_surface(seen["uvs"], seen["fuv"], 64)[0] >= 0).cpu().numpy()
    assert (~moved & chart).sum() > 0 and (~moved & ~chart).sum() > 0 and moved.sum() > 100      # there is something to fill
    for k, domain in (("chart", chart), ("map", np.ones_like(chart))):
        assert log(k) == log("off")
        line = re.search(r"Fill: (\d+) of the (\d+) texels of the (chart and gutter|map) never moved and were filled "
                         r"\((\d+) texels moved; --fill_unseen %s\)" % k, said[k])
        assert line, said[k]
        n_filled, n_domain, n_moved = int(line.group(1)), int(line.group(2)), int(line.group(4))
        assert (n_filled, n_domain, n_moved) == (int((~moved & domain).sum()), int(domain.sum()), int(moved.sum()))
        png = np.asarray(Image.open(os.path.join(folders[k], "texel_filled.png")).convert("L"))
        assert png.shape == (64, 64) and np.array_equal(png > 0, ~moved & domain) and (png > 0).sum() == n_filled
        changed = (final[k] != final["off"]).any(-1)
        assert not changed[moved].any() and not changed[~domain].any()          # moved texels and the rest of the map stay
        assert changed[~moved & chart].sum() > 0                                # unmoved chart texels took a new colour
        if k == "map":
            assert changed[~moved & ~chart].sum() > 0                           # ... and so did texels outside the chart
    # the turntable shows the filled map
    view = lambda k, i: np.asarray(Image.open(os.path.join(folders[k], "final_render", f"view_{i}.png")))
    assert any((view("chart", i) != view("off", i)).any() for i in range(12))
