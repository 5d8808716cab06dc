"""The split batch (ST3D_SPLIT_BATCH; csrc/plan.hip): a keyed loss call that finds the clean record its own runs its n images
as two groups of n / 2, the first on the caller's stream and the second on a stream of the plan's, forward and backward, with
the Grams and the loss sums over the whole batch in between.  Checked here: loss and image gradient are the one-stream plan's bit for bit along a sequence of calls whose
texture changes (both directions, and each alone); the path is taken exactly when the clean record matches; a poisoned plan
gives the same bits (no group reads what the other has yet to write); and work enqueued on the caller's stream right behind
the call sees the finished gradient without a host synchronisation.

Scenes: the cow under seeded cameras and a two-triangle quad at four distances, rendered once per module at S = 64 -- the
smallest size whose shallow convs run F(4x4,3x3) and take the flat-field and need lists (ST3D_KEEP_FORCE / ST3D_NEED_FORCE
lift the two-rounds rule) -- with n = 4 and, once, n = 8.  At S = 64 the conv3 block is 16 x 16 and has no kept lists, so one
more case runs S = 128, where conv1_2 .. conv3_3 walk their kept lists per group."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _scenes as SC
import test_gpu_epochs as TE

pytestmark = pytest.mark.gpu

WHITE = (1.0, 1.0, 1.0)
CALLS = 6
EPOCH = 31
_SWITCHES = ("ST3D_FLAT", "ST3D_FLAT_DEPTH", "ST3D_NEED_DEPTH", "ST3D_GRAPH", "ST3D_FLAT_CHECK", "ST3D_KEEP_DEPTH", "ST3D_KEEP_TILE",
             "ST3D_KEEP_SHALLOW", "ST3D_FLAT_CONV1", "ST3D_GRAM_BWD_MT", "ST3D_SPLIT_BATCH")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _env(monkeypatch, split):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ST3D_KEEP_FORCE", "1")
    monkeypatch.setenv("ST3D_NEED_FORCE", "1")
    monkeypatch.setenv("ST3D_SPLIT_BATCH", split)


# ------------------------------------------------------------------------------------------------ scenes
def _quad(n):
    """two triangles in the plane z = 0, wider than high, seen head-on from n distances: it covers a centred rectangle that
    shrinks from view to view"""
    verts = np.array([[-1.0, -0.6, 0], [1.0, -0.6, 0], [1.0, 0.6, 0], [-1.0, 0.6, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uvs = np.array([[0.03, 0.03], [0.97, 0.03], [0.97, 0.97], [0.03, 0.97]], np.float32)
    R = np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3)).copy()
    T = np.stack([np.array([0.1 * k, -0.05 * k, 2.2 + 0.6 * k], np.float32) for k in range(n)])
    return dict(verts=verts, faces=faces, verts_uvs=uvs, faces_uvs=faces.copy()), R, T


_SCENES = {}


def _scene(name, n, S, dev):
    """-> (CALLS images (n,3,S,S): the render under CALLS textures, white bit for bit outside the coverage; cover (n,S,S) uint8)"""
    key = (name, n, S)
    if key in _SCENES:
        return _SCENES[key]
    import utils as U
    U.device = dev
    if name == "cow":
        a = SC.load_asset("cow")
        R, T = SC.random_cameras(n, seed=3)
    else:
        a, R, T = _quad(n)
    rng = np.random.default_rng(5)
    imgs, cover = [], None
    for k in range(CALLS):
        tex = (rng.random((32, 32, 3), dtype=np.float32) * 0.9).astype(np.float32)
        mesh, renderer, cams = SC.device_scene(U, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], tex, R, T, S)
        with torch.no_grad():
            colour, coverage = U.render_meshes(renderer, mesh, cams)
        cov = (coverage.reshape(n, S, S) > 0)
        if cover is None:
            cover = cov
        assert torch.equal(cov, cover)                          # the geometry stays: one epoch
        img = torch.where(cover[:, None], colour.reshape(n, 3, S, S).float(), torch.ones((), device=dev))
        imgs.append(img.contiguous())
    share = float(cover.float().mean())
    assert 0.02 < share < 0.9, share
    assert all(bool(cover[i].any()) for i in range(n))
    assert not torch.equal(imgs[0], imgs[1])
    _SCENES[key] = (imgs, cover.to(torch.uint8).contiguous())
    return _SCENES[key]


def _plan(n, S, dev):
    from st3d import vgg as V
    plan = V.PerceptualPlan(TE._net(), n, S)
    g = torch.Generator().manual_seed(9)
    plan.content = torch.rand((n, 3, S, S), generator=g).to(dev)
    plan.style = torch.rand((1, 3, S, S), generator=g).to(dev).expand(n, -1, -1, -1)
    plan.set_content(plan.content, force=True)
    plan.set_style(plan.style, n, force=True)
    return plan


def _run(plan, imgs, cover, n):
    """the CALLS keyed calls -> [(loss bits, gradient bits)]"""
    out = []
    for x in imgs:
        l, g = plan.loss(x, 1e6, 1.0, batch_denom=n, need_mask=cover, flat_color=WHITE, epoch=EPOCH)
        out.append((TE._bits(l).clone(), TE._bits(g).clone()))
    torch.cuda.synchronize()
    return out


_REF = {}


def _reference(name, n, S, dev, monkeypatch):
    """the one-stream plan's results, once per scene"""
    key = (name, n, S)
    if key not in _REF:
        _env(monkeypatch, "0")
        imgs, cover = _scene(name, n, S, dev)
        plan = _plan(n, S, dev)
        try:
            _REF[key] = _run(plan, imgs, cover, n)
            assert plan.split_calls() == (0, 0)
        finally:
            plan.close()
        g = _REF[key][-1][1]
        assert bool((g != 0).any()) and all(bool(torch.isfinite(r[1].view(torch.float32)).all()) for r in _REF[key])
        assert not torch.equal(_REF[key][0][1], _REF[key][1][1])
    return _REF[key]


def _compare(name, n, S, mode, dev, monkeypatch):
    ref = _reference(name, n, S, dev, monkeypatch)
    imgs, cover = _scene(name, n, S, dev)
    _env(monkeypatch, mode)
    plan = _plan(n, S, dev)
    try:
        got = _run(plan, imgs, cover, n)
        taken = plan.split_calls()
    finally:
        plan.close()
    # the first call of the epoch fills; every later one finds the clean record its own
    assert taken == ((CALLS - 1) if mode in ("1", "fwd") else 0, (CALLS - 1) if mode in ("1", "bwd") else 0), taken
    for k, ((l1, g1), (l0, g0)) in enumerate(zip(got, ref)):
        assert torch.equal(l1, l0), (name, n, mode, "call %d: loss" % k, l1.view(torch.float32), l0.view(torch.float32))
        assert torch.equal(g1, g0), (name, n, mode, "call %d: %d gradient elements differ" % (k, int((g1 != g0).sum())))


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name,n,S,mode", [("cow", 4, 64, "1"), ("cow", 4, 64, "fwd"), ("cow", 4, 64, "bwd"), ("quad", 4, 64, "1"),
                                           ("quad", 4, 64, "fwd"), ("quad", 4, 64, "bwd"), ("cow", 8, 64, "1"), ("cow", 4, 128, "1")])
def test_split_calls_give_the_bits_of_one_stream_calls(monkeypatch, dev, name, n, S, mode):
    _compare(name, n, S, mode, dev, monkeypatch)


# ------------------------------------------------------------------------------------------------ 2. when the path is taken
def test_the_split_path_is_taken_exactly_in_clean_calls(monkeypatch, dev):
    n, S = 4, 64
    imgs, cover = _scene("cow", n, S, dev)
    _env(monkeypatch, "1")
    plan = _plan(n, S, dev)
    seen = [plan.split_calls()]

    def call(k, epoch=EPOCH, m=n):
        plan.loss(imgs[k % CALLS][:m], 1e6, 1.0, batch_denom=n, need_mask=cover[:m], flat_color=WHITE, epoch=epoch)
        seen.append(plan.split_calls())
        return (seen[-1][0] - seen[-2][0], seen[-1][1] - seen[-2][1])

    try:
        assert seen[0] == (0, 0)
        assert call(0) == (0, 0)                    # the first call of an epoch
        assert call(1) == (1, 1)
        assert call(2) == (1, 1)
        for writer in (lambda: plan.set_content(plan.content, force=True), lambda: plan.set_style(plan.style, n, force=True),
                       lambda: plan.forward(imgs[3], upto=14), lambda: plan.loss(imgs[0], 1e6, 1.0),
                       lambda: plan.loss(imgs[0], 1e6, 1.0, need_mask=cover, flat_color=WHITE)):
            writer()
            assert plan.split_calls() == seen[-1]   # none of them splits ...
            assert call(3) == (0, 0)                # ... and each clears the clean record
            assert call(4) == (1, 1)
        assert call(0, epoch=EPOCH + 1) == (0, 0)   # a new epoch
        assert call(1, epoch=EPOCH + 1) == (1, 1)
        assert call(2) == (0, 0)                    # back: the buffers hold the other epoch's call
        assert call(3) == (1, 1)
        for m in (3, 2):                            # odd, and under four
            assert call(0, m=m) == (0, 0)
            assert call(1, m=m) == (0, 0)
            assert call(2, m=m) == (0, 0)
        assert call(0) == (0, 0)
        assert call(1) == (1, 1)
        plan.profile(True)                          # profiling brackets one stream
        assert call(2) == (0, 0)
        assert call(3) == (0, 0)
        plan.profile(False)
        assert call(4) == (1, 1)
        torch.cuda.synchronize()
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------ 3. poisoned buffers
_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import pytest, torch
import test_gpu_split_batch as T
mp = pytest.MonkeyPatch()
try:
    T._compare("cow", 4, 64, "1", torch.device("cuda:0"), mp)
finally:
    mp.undo()
print("child ok")
"""


def test_the_sequence_on_poisoned_buffers():
    """ST3D_POISON_PLAN=1 in a fresh child: every plan buffer starts as NaN / -1, so a group that read a slice before its own
    chain (or the epoch's first call) wrote it would change the result"""
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here] + [p for p in sys.path if p]
    env = dict(os.environ)
    for k in _SWITCHES:
        env.pop(k, None)
    env.update(ST3D_POISON_PLAN="1")
    p = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, f"exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"


# ------------------------------------------------------------------------------------------------ 4. the caller's stream
@pytest.mark.parametrize("side", [False, True])
def test_work_enqueued_behind_the_call_sees_the_finished_gradient(monkeypatch, dev, side):
    """no host synchronisation between the calls and the copies: on the default stream, and on a stream of the caller's own"""
    n, S = 4, 64
    ref = _reference("cow", n, S, dev, monkeypatch)
    imgs, cover = _scene("cow", n, S, dev)
    _env(monkeypatch, "1")
    plan = _plan(n, S, dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream() if side else torch.cuda.current_stream()
    copies = []
    try:
        with torch.cuda.stream(stream):
            for x in imgs:
                l, g = plan.loss(x, 1e6, 1.0, batch_denom=n, need_mask=cover, flat_color=WHITE, epoch=EPOCH)
                copies.append((l.clone(), g.clone()))           # enqueued on the caller's stream, right behind the call
                g.zero_()                                       # (and the buffer is gone before the next call starts)
        stream.synchronize()
        assert plan.split_calls() == (CALLS - 1, CALLS - 1)
    finally:
        torch.cuda.synchronize()
        plan.close()
    for k, ((l1, g1), (l0, g0)) in enumerate(zip(copies, ref)):
        assert torch.equal(TE._bits(l1), l0), "call %d: loss" % k
        assert torch.equal(TE._bits(g1), g0), "call %d: %d gradient elements differ" % (k, int((TE._bits(g1) != g0).sum()))
