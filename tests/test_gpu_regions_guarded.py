"""st3d_region_planes and one whole compute_region_style_loss call between guard zones (tests/_guarded.py): every buffer
the wrappers of st3d.ops and st3d.regions allocate sits between two zones of a known byte pattern.  Nothing is written
outside the outputs, no output element keeps what its memory held before, no scratch is read before it is written: the
bits are the same under both patterns and in a plain run."""
import numpy as np
import pytest
import torch

import _guarded as G
import _regionsref as RR
import test_gpu_regions as TR

pytestmark = pytest.mark.gpu

MODULES = ("st3d.ops", "st3d.regions")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import ops as o
    return o


@pytest.fixture(scope="module")
def RG():
    from st3d import regions
    return regions


@pytest.mark.parametrize("S,Rn", [(64, 2), (64, 8), (24, 3)])
def test_region_planes_between_guard_zones(dev, ops, RG, S, Rn):
    """S = 24: partly idle tiles and dropped rows / columns; R = 8: every LDS row in use"""
    p2f, a = TR.cow_fragments(dev, ops, S)
    lab = TR.cow_labels(RG, a, Rn)
    lab_d, _ = RG.check_face_regions(lab, len(lab), device=dev)

    def run():
        planes, sums = RG.region_planes(p2f, lab_d, Rn)
        return {"planes": planes, "sums": sums}

    out = G.compare_ab(run, modules=MODULES)
    q_ref, s_ref = RR.planes_ref(p2f.cpu().numpy(), lab, Rn)
    assert np.array_equal(out["sums"].cpu().numpy().view(np.int32), s_ref.view(np.int32))
    for r in range(Rn):
        for l in range(5):
            assert np.array_equal(out[f"planes[{r}][{l}]"].cpu().numpy().view(np.int32), q_ref[r][l].view(np.int32)), (r, l)


def test_a_whole_region_loss_call_between_guard_zones(dev, ops, RG):
    import losses as L
    from st3d import vgg as V
    S, Rn = 64, 2
    vgg = V.get_vgg(seed=0, device=dev)
    p2f, lab, lab_d, cur, styles = TR._cow_case(dev, ops, RG, vgg, S, Rn)
    content, sd, cd = cur.clone().to(dev), styles.to(dev), cur.to(dev)

    def run():
        leaf = cd.clone().requires_grad_(True)
        loss = L.compute_region_style_loss(leaf, content, sd, p2f, lab_d, vgg, TR.SW, TR.CW, region_weights=(1.0, 0.5))
        loss.backward()
        return {"parts": loss.parts, "grad": leaf.grad}

    # parts is the Function's clone of the loss slots and .grad is autograd's: the plan backward's output or its copy
    out = G.compare_ab(run, modules=MODULES, own=lambda o: [o["parts"], o["grad"]])
    assert bool(torch.isfinite(out["parts"]).all()) and bool(torch.isfinite(out["grad"]).all()) and float(out["grad"].abs().max()) > 0
