"""Every wrapper of st3d/fill.py between guard zones (tests/_guarded.py): no write outside its outputs, no read of memory it did
not write (the workspace above all), and the same bits under both fill patterns and in a plain run."""
import numpy as np
import pytest
import torch

import _fillref as FR
import _guarded as G

pytestmark = pytest.mark.gpu
MODULES = ("st3d.fill",)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("tail", ["1", "0"])
def test_every_wrapper_between_guard_zones(dev, monkeypatch, tail):
    from st3d import fill
    monkeypatch.setenv("ST3D_FILL_TAIL", tail)
    rng = np.random.default_rng(11)
    # odd sides: the last workgroup of every launch is partly idle; (257, 131) runs a plain pull launch before the tail
    for H, W in ((1, 1), (1, 2), (33, 17), (129, 127), (257, 131)):
        tex = rng.random((H, W, 3), dtype=np.float32)
        valid = (rng.random((H, W)) < 0.3).astype(np.uint8)
        valid[0, 0] = 0
        valid[H - 1, W - 1] = 1
        domain = (rng.random((H, W)) < 0.6).astype(np.uint8)
        d_tex, d_valid, d_domain = _t(tex, dev), _t(valid, dev), _t(domain, dev)
        for dom, d_dom in ((None, None), (domain, d_domain)):
            out = G.compare_ab(lambda: dict(zip(("filled", "count"), fill.push_pull(d_tex, d_valid, d_dom))), modules=MODULES)
            want, n, _ = FR.push_pull(tex, valid, dom, dtype=np.float32)
            assert int(out["count"]) == n
            assert np.array_equal(out["filled"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        none = G.compare_ab(lambda: dict(zip(("filled", "count"), fill.push_pull(d_tex, torch.zeros_like(d_valid)))),
                            modules=MODULES)
        assert int(none["count"]) == 0 and torch.equal(none["filled"], d_tex)      # nothing valid: the workspace's zeros reach nothing
        original = d_tex.clone()
        original[d_valid == 0] += 1.0                       # the texels with valid = 0 are the ones that "moved"
        moved = G.compare_ab(lambda: {"moved": fill.moved_texels(d_tex, original)}, modules=MODULES)
        assert torch.equal(moved["moved"], (d_valid == 0).to(torch.uint8))
        both = G.compare_ab(lambda: dict(zip(("filled", "count"), fill.fill_unseen(d_tex, original, d_domain))), modules=MODULES)
        want, n, _ = FR.push_pull(tex, 1 - valid, domain, dtype=np.float32)
        assert int(both["count"]) == n and np.array_equal(both["filled"].cpu().numpy().view(np.uint32), want.view(np.uint32))
