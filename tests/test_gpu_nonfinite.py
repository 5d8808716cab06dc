"""NaN / Inf through the VGG, Gram, loss and Adam kernels, and the planted value as a tracer of each kernel's reads.

Per case: launch on clean inputs, plant bad in {NaN, +Inf, -Inf} at one element, launch again, and compare with the fp64
PyTorch reference of the same op on the poisoned inputs (CPU):
  must <= kernel : every output the reference makes non-finite is non-finite in the kernel (a diverged run fails as
                   loudly as in the reference: torch.relu(nan) = nan, threshold_backward lets the gradient through a NaN)
  kernel <= may  : every non-finite kernel output lies in the op's dependency footprint (tests/_footprints.py)
  outside may    : every output equals the clean launch bit for bit (fixed summation orders), so a read outside the
                   footprint -- a stale ring stage, a neighbouring tile's halo, another image or slot, padding read from
                   memory -- shows even where a zero weight or a cancelling sum hides it from the value tests.
NaN and Inf classes need not match: a Winograd transform turns +-Inf into NaN.  A NaN or +Inf in a pure gate operand opens
the gate and -Inf closes it: the launch is then bitwise the launch with a finite open (1) or closed (0) gate there.

The fp64 references of the convolutions are computed on the rows the planted element reaches (exactly: the real
neighbouring rows, zero padding only at the image border); every other output of the reference takes finite inputs only.
ST3D_DIAG_LIB runs the same file against another build of the library."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _footprints as fp

pytestmark = pytest.mark.gpu

BADS = [float("nan"), float("inf"), float("-inf")]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from st3d import _lib, ops as o
    if os.environ.get("ST3D_DIAG_LIB"):          # the same tests against another build of the library
        _lib.SO_PATH = os.path.abspath(os.environ["ST3D_DIAG_LIB"])
    return o


def _where(m):
    i = m.nonzero()
    return f"{int(m.sum())} elements, first at {tuple(i[0].tolist())}" if i.shape[0] else "none"


def _check(name, clean, dirty, ref, may):
    """The three assertions of the module docstring.  ref: fp64 reference on the poisoned inputs (None: nothing must be
    non-finite); may: bool footprint."""
    clean, dirty = clean.detach().cpu(), dirty.detach().cpu()
    assert clean.shape == dirty.shape == may.shape, (name, clean.shape, dirty.shape, may.shape)
    assert torch.isfinite(clean).all(), f"{name}: the clean launch is not finite"
    bad = ~torch.isfinite(dirty)
    if ref is not None:
        miss = ~torch.isfinite(ref.cpu()) & ~bad
        assert not miss.any(), f"{name}: must <= kernel: reference non-finite, kernel finite: {_where(miss)}"
    stray = bad & ~may
    assert not stray.any(), f"{name}: kernel <= may: non-finite outside the footprint: {_where(stray)}"
    out = ~may
    diff = out & (clean.view(torch.int32) != dirty.view(torch.int32))
    assert not diff.any(), f"{name}: outside the footprint the launch differs from the clean one: {_where(diff)}"


def _gate_value(bad):
    return 0.0 if bad <= 0 else 1.0          # threshold_backward: NaN and +Inf open the gate, -Inf closes it


def _check_gate(name, run, t, idx, bad, clean):
    """Pure gate operand t: poisoned at idx, the launch must be bitwise the launch with the equivalent finite gate."""
    tb = t.clone()
    tb[idx] = bad
    dirty = run(tb)
    tb[idx] = _gate_value(bad)
    want = run(tb)
    assert torch.isfinite(dirty).all(), f"{name}: a gate operand leaked into the values"
    assert torch.equal(dirty.view(torch.int32), want.view(torch.int32)), \
        f"{name}: NaN / Inf gate != finite gate {_gate_value(bad)}: {_where(dirty.cpu() != want.cpu())}"
    assert clean is None or torch.isfinite(clean).all()


def _conv_rows(xi, w, b, y0, y1):
    """Exact fp64 rows [y0, y1) of the 3x3 / pad-1 convolution of one image xi (C, H, W)."""
    H = xi.shape[1]
    lo, hi = y0 - 1, y1 + 1
    part = F.pad(xi[:, max(lo, 0):min(hi, H)], (0, 0, max(0, -lo), max(0, hi - H)))
    return F.conv2d(part[None], w, b, padding=(0, 1))[0]


def _conv_ref(x, w, b, n, y, relu, pool=False):
    """fp64 reference of conv (+ ReLU) (+ 2x2 max pool) of image n of x, exact on the rows a bad element at row y reaches,
    zero elsewhere (finite there).  x on the CPU, any dtype."""
    N, _, H, W = x.shape
    y0, y1 = max(y - 1, 0), min(y + 2, H)
    if pool:
        y0, y1 = y0 // 2 * 2, min((y1 + 1) // 2 * 2, H // 2 * 2)
    r = _conv_rows(x[n].double(), w.double(), None if b is None else b.double(), y0, y1)
    if relu:
        r = torch.relu(r)
    shape = (N, w.shape[0], H, W)
    if pool:
        r = F.max_pool2d(r[None], 2, 2)[0]
        y0, y1 = y0 // 2, y1 // 2
        shape = (N, w.shape[0], H // 2, W // 2)
    out = torch.zeros(shape, dtype=torch.float64)
    out[n, :, y0:y1] = r
    return out


def _plants(N, C, H, W):
    """Where kernels go wrong: image borders (row 0, row H-1, column W-1), y % 4 in {0, 3}, both sides of the 32- and
    64-pixel workgroup-step boundaries, the first / last channel of a 16-channel stage and channel C-1; image 1 of N."""
    n = 1 if N > 1 else 0
    pts = [(n, 0, 0, 0), (n, C - 1, H - 1, W - 1), (n, min(15, C - 1), min(3, H - 1), min(31, W - 1))]
    if W > 64:
        pts.append((n, min(16, C - 1), min(4, H - 1), 64))
        pts.append((n, C - 1, H // 2, 63))
    elif W > 32:
        pts.append((n, min(16, C - 1), min(4, H - 1), 32))
    return pts


def _launch_pair(run, x, idx, bad):
    xb = x.clone()
    xb[idx] = bad
    return run(xb), xb


# ---------------------------------------------------------------------------- direct conv / pool
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(3, 3, 64, 40, 68), (3, 64, 128, 12, 80)])
def test_conv3x3_fwd_dgrad_and_pool(dev, ops, N, Cin, Cout, H, W):
    """Cin 3 = the VALU conv1_1 kernels, Cin 64 = the MFMA kernels; forward with and without ReLU, input gradient (bad
    value in gy, and in the ReLU gate act), the unpool input gradient, and the max pool."""
    g = torch.Generator().manual_seed(Cin + W)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    wf, wd = ops.conv3x3_pack(w.to(dev))
    xd, bd = x.to(dev), b.to(dev)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()            # input gradient = conv with the flipped, transposed filter
    for relu in (True, False):
        run = lambda t: ops.conv3x3_fwd(t, wf, bd, Cout, relu=relu)              # noqa: E731
        clean = run(xd)
        for (n, c, y, xx) in _plants(N, Cin, H, W):
            for bad in BADS:
                dirty, xb = _launch_pair(run, xd, (n, c, y, xx), bad)
                _check(f"conv fwd relu={relu} {(n, c, y, xx)} {bad}", clean, dirty,
                       _conv_ref(xb.cpu(), w, b, n, y, relu), fp.conv3x3(clean.shape, n, y, xx))
    act = ops.conv3x3_fwd(xd, wf, bd, Cout, relu=True)
    gy = torch.randn(N, Cout, H, W, generator=g).to(dev)
    run = lambda t: ops.conv3x3_dgrad(t, act, wd, Cin)                           # noqa: E731
    clean = run(gy)
    for (n, c, y, xx) in _plants(N, Cout, H, W):
        for bad in BADS:
            dirty, gb = _launch_pair(run, gy, (n, c, y, xx), bad)
            gcpu = gb.double().cpu()
            ref = _conv_ref(torch.where(act.cpu() <= 0, torch.zeros_like(gcpu), gcpu), wt, None, n, y, False)
            _check(f"conv dgrad gy {(n, c, y, xx)} {bad}", clean, dirty, ref, fp.conv3x3(clean.shape, n, y, xx))
            _check_gate(f"conv dgrad act {(n, c, y, xx)} {bad}", lambda a: ops.conv3x3_dgrad(gy, a, wd, Cin), act,
                        (n, c, y, xx), bad, clean)
    if Cin >= 64:
        # max pool and the unpool input gradient
        pooled, idx = ops.maxpool2x2(act)
        for (n, c, y, xx) in _plants(N, Cout, H, W):
            for bad in BADS:
                pb, ab = _launch_pair(lambda t: ops.maxpool2x2(t)[0], act, (n, c, y, xx), bad)
                _check(f"maxpool {(n, c, y, xx)} {bad}", pooled, pb, F.max_pool2d(ab.double().cpu(), 2, 2),
                       fp.pool2x2(fp.element(act.shape, n, c, y, xx)))
        gp = torch.randn(pooled.shape, generator=g).to(dev)
        run = lambda t: ops.conv3x3_dgrad_unpool(t, idx, pooled, wd, Cin)          # noqa: E731
        clean = run(gp)
        for (n, c, yp, xp) in _plants(N, Cout, H // 2, W // 2):
            k = int(idx[n, c, yp, xp])
            y, xx = 2 * yp + (k >> 1), 2 * xp + (k & 1)
            for bad in BADS:
                dirty, gb = _launch_pair(run, gp, (n, c, yp, xp), bad)
                up = torch.zeros(act.shape, dtype=torch.float64)
                if float(pooled[n, c, yp, xp]) > 0:
                    up[n, c, y, xx] = bad
                _check(f"conv dgrad_unpool {(n, c, yp, xp)} {bad}", clean, dirty, _conv_ref(up, wt, None, n, y, False),
                       fp.conv3x3(clean.shape, n, y, xx))
                _check_gate(f"conv dgrad_unpool pooled {(n, c, yp, xp)} {bad}",
                            lambda p: ops.conv3x3_dgrad_unpool(gp, idx, p, wd, Cin), pooled, (n, c, yp, xp), bad, clean)


# ---------------------------------------------------------------------------- F(2x2,3x3)
@pytest.mark.parametrize("N,Cin,Cout,H,W", [(3, 64, 64, 16, 128), (2, 128, 64, 10, 40),
                                             (3, 64, 64, 256, 128)])       # more workgroup tiles than CUs
def test_wino_fwd_and_dgrads(dev, ops, N, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(Cin + H + W)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    uf, ud = ops.wino_pack(w.to(dev))
    xd, bd = x.to(dev), b.to(dev)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    plants = _plants(N, Cin, H, W)
    for relu in (True, False):
        run = lambda t: ops.wino_fwd(t, uf, bd, Cout, relu=relu)                  # noqa: E731
        clean = run(xd)
        for (n, c, y, xx) in plants:
            for bad in BADS:
                dirty, xb = _launch_pair(run, xd, (n, c, y, xx), bad)
                _check(f"wino fwd relu={relu} {(n, c, y, xx)} {bad}", clean, dirty, _conv_ref(xb.cpu(), w, b, n, y, relu),
                       fp.conv3x3(clean.shape, n, y, xx, 2))
    # fused pool
    yc, pc, ic = ops.wino_fwd(xd, uf, bd, Cout, relu=True, pool=True)
    for (n, c, y, xx) in plants:
        for bad in BADS:
            xb = xd.clone()
            xb[n, c, y, xx] = bad
            yb, pb, ib = ops.wino_fwd(xb, uf, bd, Cout, relu=True, pool=True)
            may = fp.conv3x3(yc.shape, n, y, xx, 2)
            _check(f"wino fwd+pool full {(n, c, y, xx)} {bad}", yc, yb, _conv_ref(xb.cpu(), w, b, n, y, True), may)
            _check(f"wino fwd+pool pooled {(n, c, y, xx)} {bad}", pc, pb, _conv_ref(xb.cpu(), w, b, n, y, True, pool=True),
                   fp.pool2x2(may))
            assert torch.equal(ic.cpu()[~fp.pool2x2(may)], ib.cpu()[~fp.pool2x2(may)])
    # input gradients: gy (value), act / pooled (gates), out_gate (gate; value with add_target), add_target (value)
    act, pooled, pidx = ops.wino_fwd(xd, uf, bd, Cout, relu=True, pool=True)
    gy = torch.randn(N, Cout, H, W, generator=g).to(dev)
    gp = torch.randn(pooled.shape, generator=g).to(dev)
    og = torch.randn(N, Cin, H, W, generator=g).to(dev)
    tgt = torch.randn(N, Cin, H, W, generator=g).to(dev)
    coef = 0.37
    for (n, c, y, xx) in _plants(N, Cout, H, W)[:3]:
        for bad in BADS:
            gb = gy.clone()
            gb[n, c, y, xx] = bad
            gcpu = gb.double().cpu()
            gated = torch.where(act.cpu() <= 0, torch.zeros_like(gcpu), gcpu)
            ref = _conv_ref(gated, wt, None, n, y, False)
            may = fp.conv3x3(gy.shape[:1] + (Cin,) + gy.shape[2:], n, y, xx, 2)
            _check(f"wino dgrad gy {(n, c, y, xx)} {bad}", ops.wino_dgrad(gy, act, ud, Cin), ops.wino_dgrad(gb, act, ud, Cin),
                   ref, may)
            pre = lambda t: torch.where(act > 0, t, torch.zeros_like(t))             # noqa: E731  (the content term rides on pre-gated input)
            clean = ops.wino_dgrad_chain(pre(gy), ud, Cin, out_gate=og, add_target=tgt, add_coef=coef)
            dirty = ops.wino_dgrad_chain(pre(gb), ud, Cin, out_gate=og, add_target=tgt, add_coef=coef)
            ogc = og.double().cpu()
            ref_c = torch.where(ogc <= 0, torch.zeros_like(ref), ref + coef * (ogc - tgt.double().cpu()))
            _check(f"wino dgrad_chain gy {(n, c, y, xx)} {bad}", clean, dirty, ref_c, may)
            _check_gate(f"wino dgrad act {(n, c, y, xx)} {bad}", lambda a: ops.wino_dgrad(gy, a, ud, Cin), act,
                        (n, c, y, xx), bad, None)
            _check_gate(f"wino dgrad_chain act {(n, c, y, xx)} {bad}",
                        lambda a: ops.wino_dgrad_chain(gy, ud, Cin, act=a, out_gate=og), act, (n, c, y, xx), bad, None)
    gy_pre = torch.where(act > 0, gy, torch.zeros_like(gy))
    for (n, c, y, xx) in _plants(N, Cin, H, W)[:3]:
        for bad in BADS:
            e = (n, c, y, xx)
            _check_gate(f"wino dgrad_chain out_gate {e} {bad}", lambda o: ops.wino_dgrad_chain(gy, ud, Cin, act=act, out_gate=o),
                        og, e, bad, None)
            clean = ops.wino_dgrad_chain(gy_pre, ud, Cin, out_gate=og, add_target=tgt, add_coef=coef)
            base = clean.double().cpu()
            for which in ("out_gate", "add_target"):
                ob, tb = og.clone(), tgt.clone()
                (ob if which == "out_gate" else tb)[e] = bad
                dirty = ops.wino_dgrad_chain(gy_pre, ud, Cin, out_gate=ob, add_target=tb, add_coef=coef)
                # elementwise part of the reference at the poisoned element (the convolution term there is finite)
                o_, t_ = float(ob[e]), float(tb[e])
                ref = torch.zeros_like(base)
                ref[e] = 0.0 if o_ <= 0 else base[e] + coef * (o_ - t_)
                _check(f"wino dgrad_chain {which} {e} {bad}", clean, dirty, ref, fp.element(clean.shape, *e))
    for (n, c, yp, xp) in _plants(N, Cout, H // 2, W // 2)[:3]:
        k = int(pidx[n, c, yp, xp])
        y, xx = 2 * yp + (k >> 1), 2 * xp + (k & 1)
        may = fp.conv3x3((N, Cin, H, W), n, y, xx, 2)
        for bad in BADS:
            gb = gp.clone()
            gb[n, c, yp, xp] = bad
            up = torch.zeros(act.shape, dtype=torch.float64)
            if float(pooled[n, c, yp, xp]) > 0:
                up[n, c, y, xx] = bad
            ref = _conv_ref(up, wt, None, n, y, False)
            _check(f"wino dgrad_unpool {(n, c, yp, xp)} {bad}", ops.wino_dgrad_unpool(gp, pidx, pooled, ud, Cin),
                   ops.wino_dgrad_unpool(gb, pidx, pooled, ud, Cin), ref, may)
            _check(f"wino dgrad_chain pool {(n, c, yp, xp)} {bad}", ops.wino_dgrad_chain(gp, ud, Cin, pool_idx=pidx, pooled=pooled),
                   ops.wino_dgrad_chain(gb, ud, Cin, pool_idx=pidx, pooled=pooled), ref, may)
            _check_gate(f"wino dgrad_unpool pooled {(n, c, yp, xp)} {bad}",
                        lambda p: ops.wino_dgrad_unpool(gp, pidx, p, ud, Cin), pooled, (n, c, yp, xp), bad, None)


# ---------------------------------------------------------------------------- F(4x4,3x3)
W43_CASES = [(3, 64, 64, 8, 128),         # 4 x 64-pixel workgroup steps (TC = 16)
             (3, 64, 128, 16, 96)]      # 8 x 32-pixel steps (TC = 8)


@pytest.mark.parametrize("N,Cin,Cout,H,W,slots", [c + (s,) for c in W43_CASES for s in ("", "1", "4")] +
                         [(1, 64, 64, 128, 128, "")])      # more tiles than CUs
def test_wino43_fwd_and_chain_dgrad(dev, ops, monkeypatch, N, Cin, Cout, H, W, slots):
    """slots "1" / "4": one persistent workgroup walks the tiles of several images across the poisoned one."""
    if slots:
        monkeypatch.setenv("ST3D_W43_SLOTS", slots)
    g = torch.Generator().manual_seed(Cin + Cout + H)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (Cin * 9)) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    uf, ud = ops.wino43_pack(w.to(dev))
    xd, bd = x.to(dev), b.to(dev)
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    plants = _plants(N, Cin, H, W)
    for relu in (True, False):
        run = lambda t: ops.wino43_fwd(t, uf, bd, Cout, relu=relu)                # noqa: E731
        clean = run(xd)
        for (n, c, y, xx) in plants:
            for bad in BADS:
                dirty, xb = _launch_pair(run, xd, (n, c, y, xx), bad)
                _check(f"wino43 fwd relu={relu} {(n, c, y, xx)} {bad}", clean, dirty, _conv_ref(xb.cpu(), w, b, n, y, relu),
                       fp.conv3x3(clean.shape, n, y, xx, 4))
    _, pc, ic = ops.wino43_fwd(xd, uf, bd, Cout, relu=True, pool=True, keep_full=False)
    for (n, c, y, xx) in plants:
        for bad in BADS:
            xb = xd.clone()
            xb[n, c, y, xx] = bad
            none, pb, ib = ops.wino43_fwd(xb, uf, bd, Cout, relu=True, pool=True, keep_full=False)
            may = fp.pool2x2(fp.conv3x3((N, Cout, H, W), n, y, xx, 4))
            _check(f"wino43 fwd+pool {(n, c, y, xx)} {bad}", pc, pb, _conv_ref(xb.cpu(), w, b, n, y, True, pool=True), may)
            assert none is None and torch.equal(ic.cpu()[~may], ib.cpu()[~may])
    # chain input gradient: plain, fused unpool, producer-side out_gate, out_gate + add_target
    act = ops.wino43_fwd(xd, uf, bd, Cout, relu=True)
    gy = torch.where(act > 0, torch.randn(act.shape, generator=g).to(dev), torch.zeros_like(act))
    og = torch.randn(N, Cin, H, W, generator=g).to(dev)
    tgt = torch.randn(N, Cin, H, W, generator=g).to(dev)
    coef = 0.37
    ogc, tgc = og.double().cpu(), tgt.double().cpu()
    for (n, c, y, xx) in _plants(N, Cout, H, W):
        may = fp.conv3x3((N, Cin, H, W), n, y, xx, 4)
        for bad in BADS:
            gb = gy.clone()
            gb[n, c, y, xx] = bad
            ref = _conv_ref(gb.cpu(), wt, None, n, y, False)
            for kw, r in (({}, ref), ({"out_gate": og}, torch.where(ogc <= 0, torch.zeros_like(ref), ref)),
                          ({"out_gate": og, "add_target": tgt, "add_coef": coef},
                           torch.where(ogc <= 0, torch.zeros_like(ref), ref + coef * (ogc - tgc)))):
                _check(f"wino43 chain {sorted(kw)} gy {(n, c, y, xx)} {bad}", ops.wino43_dgrad_chain(gy, ud, Cin, **kw),
                       ops.wino43_dgrad_chain(gb, ud, Cin, **kw), r, may)
    for (n, c, y, xx) in _plants(N, Cin, H, W)[:3]:
        for bad in BADS:
            _check_gate(f"wino43 chain out_gate {(n, c, y, xx)} {bad}", lambda o: ops.wino43_dgrad_chain(gy, ud, Cin, out_gate=o),
                        og, (n, c, y, xx), bad, None)
    gp = torch.randn(N, Cout, H // 2, W // 2, generator=g).to(dev)
    pidx = torch.randint(0, 4, gp.shape, dtype=torch.uint8, generator=g).to(dev)
    for (n, c, yp, xp) in _plants(N, Cout, H // 2, W // 2):
        k = int(pidx[n, c, yp, xp])
        y, xx = 2 * yp + (k >> 1), 2 * xp + (k & 1)
        for bad in BADS:
            gb = gp.clone()
            gb[n, c, yp, xp] = bad
            up = torch.zeros((N, Cout, H, W), dtype=torch.float64)
            up[n, c, y, xx] = bad
            _check(f"wino43 chain pool_idx {(n, c, yp, xp)} {bad}", ops.wino43_dgrad_chain(gp, ud, Cin, pool_idx=pidx),
                   ops.wino43_dgrad_chain(gb, ud, Cin, pool_idx=pidx), _conv_ref(up, wt, None, n, y, False),
                   fp.conv3x3((N, Cin, H, W), n, y, xx, 4))


# ---------------------------------------------------------------------------- conv1_1 backward (tap0)
@pytest.mark.parametrize("N,H,W", [(3, 40, 52), (3, 17, 22)])
def test_conv1_bwd(dev, ops, N, H, W):
    """gx = conv1_1^T(gate(gy + coef * D act)); bad value in gy, act (gate and Gram operand) and D."""
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(N, 3, H, W, generator=g, dtype=torch.float64)
    w = (torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5).double()
    b = (torch.randn(64, generator=g) * 0.1).double()
    act = torch.relu(F.conv2d(x, w, b, padding=1))
    gy = torch.randn(act.shape, generator=g, dtype=torch.float64)
    D = torch.randn(N, 64, 64, generator=g, dtype=torch.float64)
    D = 0.5 * (D + D.transpose(1, 2))
    coef = 0.37
    _, wd = ops.conv3x3_pack(w.float().to(dev))

    def ref(gy_, act_, D_):
        t = gy_ + coef * torch.bmm(D_, act_.flatten(2)).reshape(act_.shape)
        t = torch.where(act_ <= 0, torch.zeros_like(t), t)
        return F.conv_transpose2d(t, w, padding=1)

    args = [t.float().to(dev).contiguous() for t in (gy, act, D)]
    clean = ops.conv1_bwd(args[0], args[1], args[2], coef, wd)
    for which in range(3):
        base = args[which]
        for bad in BADS:
            for e in ([(1, 0, 0, 0), (1, 63, H - 1, W - 1), (1, 15, 3, W // 2)] if which < 2 else
                      [(1, 0, 0), (1, 63, 63)]):
                if which == 1 and float(act[e]) <= 0:
                    continue                          # a zero activation planted: the Gram term decides, covered by D
                t = base.clone()
                t[e] = bad
                a = list(args)
                a[which] = t
                dirty = ops.conv1_bwd(a[0], a[1], a[2], coef, wd)
                r = ref(*[v.double().cpu() for v in a])
                if which < 2:
                    may = fp.conv3x3(clean.shape, e[0], e[2], e[3])
                else:
                    may = torch.zeros(clean.shape, dtype=torch.bool)
                    may[e[0]] = True
                _check(f"conv1_bwd {['gy', 'act', 'D'][which]} {e} {bad}", clean, dirty, r, may)


# ---------------------------------------------------------------------------- Gram
@pytest.mark.parametrize("B,C,H,W", [(3, 64, 40, 40), (3, 128, 17, 19), (2, 512, 8, 8)])
def test_gram_fwd_and_bwd(dev, ops, B, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    f = torch.relu(torch.randn(B, C, H, W, generator=g)).to(dev)
    D = torch.randn(B, C, C, generator=g)
    D = (0.5 * (D + D.transpose(1, 2))).to(dev).contiguous()      # gram_bwd_gated takes D = G - S, symmetric
    base = torch.randn(B, C, H, W, generator=g).to(dev)
    HW = H * W
    clean = ops.gram_fwd(f)
    cb = {k: ops.gram_bwd(D, f, 0.3, out=base.clone() if k == "acc" else None, gated=k == "gated") for k in ("plain", "acc", "gated")}
    for (n, c, p) in [(1, 0, 0), (1, C - 1, HW - 1), (1, 15, HW - 3), (B - 1, 16, HW // 2)]:
        e = (n, c, p // W, p % W)
        for bad in BADS:
            fb = f.clone()
            fb[e] = bad
            fd = fb.double().cpu().flatten(2)
            _check(f"gram {e} {bad}", clean, ops.gram_fwd(fb), torch.bmm(fd, fd.transpose(1, 2)), fp.gram(B, C, n, c))
            Dd = D.double().cpu()
            for k, out in cb.items():
                r = 0.3 * torch.bmm(Dd, fd).reshape(B, C, H, W)
                if k == "acc":
                    r = r + base.double().cpu()
                if k == "gated":
                    r = torch.where(fb.double().cpu() <= 0, torch.zeros_like(r), r)
                dirty = ops.gram_bwd(D, fb, 0.3, out=base.clone() if k == "acc" else None, gated=k == "gated")
                _check(f"gram_bwd {k} F {e} {bad}", out, dirty, r, fp.gram_bwd_feat(f.shape, n, p))
            b2 = (c * 7 + 3) % C
            Db = D.clone()
            Db[n, c, b2] = Db[n, b2, c] = bad                           # stays symmetric: rows c and b2
            for k, out in cb.items():
                r = 0.3 * torch.bmm(Db.double().cpu(), f.double().cpu().flatten(2)).reshape(B, C, H, W)
                if k == "gated":
                    r = torch.where(f.double().cpu() <= 0, torch.zeros_like(r), r)
                dirty = ops.gram_bwd(Db, f, 0.3, out=base.clone() if k == "acc" else None, gated=k == "gated")
                _check(f"gram_bwd {k} D {(n, c, b2)} {bad}", out, dirty, r,
                       fp.gram_bwd_D(f.shape, n, c) | fp.gram_bwd_D(f.shape, n, b2))


def test_gram_fwd_multi_keeps_other_layers_and_images_clean(dev, ops):
    g = torch.Generator().manual_seed(7)
    shapes = [(3, 64, 64, 64), (3, 128, 32, 32), (3, 256, 16, 16), (3, 512, 8, 8), (3, 512, 4, 4)]
    feats = [torch.relu(torch.randn(sh, generator=g)).to(dev) for sh in shapes]
    clean = ops.gram_fwd_multi(feats)
    for li, (B, C, H, W) in enumerate(shapes):
        for (c, p) in [(0, 0), (C - 1, H * W - 1)]:
            for bad in BADS:
                fs = list(feats)
                fs[li] = feats[li].clone()
                fs[li][1, c, p // W, p % W] = bad
                dirty = ops.gram_fwd_multi(fs)
                for lj, (gc, gd) in enumerate(zip(clean, dirty)):
                    Cj = shapes[lj][1]
                    may = fp.gram(3, Cj, 1, c) if lj == li else torch.zeros((3, Cj, Cj), dtype=torch.bool)
                    fd = fs[lj].double().cpu().flatten(2)
                    _check(f"gram multi layer {li} -> {lj} {(c, p)} {bad}", gc, gd, torch.bmm(fd, fd.transpose(1, 2)), may)


# ---------------------------------------------------------------------------- losses, gates, Adam
def _scalar_nonfinite(name, got, ref):
    got, ref = float(got.reshape(-1)[0]), float(ref)
    assert math.isfinite(got) == math.isfinite(ref), f"{name}: kernel {got} vs reference {ref}"


def test_losses_adam_and_axpy(dev, ops):
    """Scalar losses are non-finite iff the fp64 reference expression is (NaN * 0 = NaN: a masked-out NaN still poisons
    masked_mse and tv_loss); gradients and Adam follow the elementwise rule."""
    g = torch.Generator().manual_seed(11)
    B, S = 3, 24
    r = torch.rand(B, 3, S, S, generator=g, dtype=torch.float64)
    t = torch.rand(B, 3, S, S, generator=g, dtype=torch.float64)
    m = (torch.rand(B, 1, S, S, generator=g) > 0.4).double()
    m[1, 0, 0, 0], m[1, 0, S - 1, S - 1] = 0.0, 1.0
    rd, td, md = (v.float().to(dev) for v in (r, t, m))
    plants = [(1, 0, 0, 0), (1, 2, S - 1, S - 1), (1, 1, 5, 7)]
    l0, g0 = ops.masked_mse(rd, td, md)
    s0, d0 = ops.sqdiff_sum(rd, td, scale=0.5, want_diff=True)
    tv0, tg0 = ops.tv_loss(rd, md)
    v = (torch.randn(5000, generator=g) * 0.7 + 0.5).double()
    rl0, rg0 = ops.range_loss(v.float().to(dev))
    for e in plants:
        for bad in BADS:
            rb = r.clone()
            rb[e] = bad
            rbd = rb.float().to(dev)
            rq = rb.clone().requires_grad_(True)
            ref = F.mse_loss(rq * m, t * m)
            ref.backward()
            lb, gb = ops.masked_mse(rbd, td, md)
            _scalar_nonfinite(f"masked_mse {e} {bad}", lb, ref.detach())
            _check(f"masked_mse grad {e} {bad}", g0, gb, rq.grad, fp.element(r.shape, *e))
            sb, db = ops.sqdiff_sum(rbd, td, scale=0.5, want_diff=True)
            _scalar_nonfinite(f"sqdiff_sum {e} {bad}", sb, 0.5 * ((rb - t) ** 2).sum())
            _check(f"sqdiff diff {e} {bad}", d0, db, rb - t, fp.element(r.shape, *e))
            rq = rb.clone().requires_grad_(True)
            tv = ((rq[:, :, 1:] - rq[:, :, :-1]).abs() * (m[:, :, 1:] * m[:, :, :-1])).sum() + \
                 ((rq[..., 1:] - rq[..., :-1]).abs() * (m[..., 1:] * m[..., :-1])).sum()
            tv = tv / m.sum()
            tv.backward()
            tvb, tgb = ops.tv_loss(rbd, md)
            _scalar_nonfinite(f"tv_loss {e} {bad}", tvb, tv.detach())
            n, c, y, x = e
            may = torch.zeros(r.shape, dtype=torch.bool)
            may[n, c, max(y - 1, 0):y + 2, x] = True
            may[n, c, y, max(x - 1, 0):x + 2] = True
            _check(f"tv grad {e} {bad}", tg0, tgb, rq.grad, may)
    for i in (0, 1999, 4999):
        for bad in BADS:
            vb = v.clone()
            vb[i] = bad
            vq = vb.clone().requires_grad_(True)
            ref = (torch.relu(vq - 1) + torch.relu(-vq)).sum()
            ref.backward()
            lb, gb = ops.range_loss(vb.float().to(dev))
            _scalar_nonfinite(f"range_loss {i} {bad}", lb, ref.detach())
            _check(f"range grad {i} {bad}", rg0, gb, vq.grad, fp.element(v.shape, i))
    # axpy_diff (content term; gated: a is both the value and the ReLU gate)
    n = 3000
    a = torch.relu(torch.randn(n, generator=g)).to(dev)
    bb = torch.randn(n, generator=g).to(dev)
    gbase = torch.randn(n, generator=g).to(dev)
    from st3d._lib import call, dptr, stream_ptr

    def axpy(a_, b_, gated):
        out = gbase.clone()
        call("st3d_axpy_diff_gated" if gated else "st3d_axpy_diff", dptr(a_), dptr(b_), n, 0.25, 1, dptr(out), stream_ptr())
        return out
    for gated in (False, True):
        c0 = axpy(a, bb, gated)
        for i in (0, 1234, n - 1):
            for bad in BADS:
                for which in ("a", "b"):
                    ab, b2 = a.clone(), bb.clone()
                    (ab if which == "a" else b2)[i] = bad
                    ac, bc, gc = ab.double().cpu(), b2.double().cpu(), gbase.double().cpu()
                    ref = gc + 0.25 * (ac - bc)
                    if gated:
                        ref = torch.where(ac <= 0, torch.zeros_like(ref), ref)
                    _check(f"axpy_diff gated={gated} {which} {i} {bad}", c0, axpy(ab, b2, gated), ref, fp.element((n,), i))
    # Adam: one step from a state, bad value in the gradient
    p0 = torch.randn(4000, generator=g)
    m0 = torch.randn(4000, generator=g) * 0.01
    v0 = torch.rand(4000, generator=g) * 0.01
    gr = torch.randn(4000, generator=g)

    def adam(grad):
        p, mm, vv = p0.clone().to(dev), m0.clone().to(dev), v0.clone().to(dev)
        ops.adam_step(p, grad.to(dev), mm, vv, 3, 0.01)
        return torch.stack([p, mm, vv])
    clean = adam(gr)
    for i in (0, 2047, 3999):
        for bad in BADS:
            gb = gr.clone()
            gb[i] = bad
            mr = 0.9 * m0.double() + 0.1 * gb.double()
            vr = 0.999 * v0.double() + 0.001 * gb.double() ** 2
            pr = p0.double() - 0.01 * (mr / (1 - 0.9 ** 3)) / ((vr / (1 - 0.999 ** 3)).sqrt() + 1e-8)
            may = torch.zeros((3, 4000), dtype=torch.bool)
            may[:, i] = True
            _check(f"adam {i} {bad}", clean, adam(gb), torch.stack([pr, mr, vr]), may)


# ---------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_perceptual_loss_end_to_end(dev, ops, bad):
    """One bad pixel in image 1 of 3 at 64^2: the loss is non-finite whenever the fp64 CPU restatement is, and the gradient
    of images 0 and 2 is bitwise the clean run's (the reference's Grams are per image).  Goes through st3d_plan_loss /
    st3d_plan_backward and the fused relu1_1 / conv1_1 backward."""
    import losses as L
    import utils as U
    from oracle import perceptual_ref as P
    g = torch.Generator().manual_seed(2)
    B, S = 3, 64
    cur0 = torch.rand(B, 3, S, S, generator=g)
    con = torch.rand(B, 3, S, S, generator=g).to(dev)
    sty = torch.rand(1, 3, S, S, generator=g).to(dev)
    vgg = U.get_vgg(seed=0)

    def run(img):
        cur = img.clone().to(dev).requires_grad_(True)
        loss = L.compute_perceptual_loss(cur, con, sty.expand(B, -1, -1, -1), vgg)
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), cur.grad.detach().cpu()
    l0, g0 = run(cur0)
    assert math.isfinite(l0) and torch.isfinite(g0).all()
    cb = cur0.clone()
    cb[1, 1, 31, 32] = bad
    l1, g1 = run(cb)
    model = P.make_vgg19_features(seed=0)
    with torch.no_grad():
        ref = P.perceptual_loss_ref(cb.double(), con.cpu().double(), sty.cpu().double().expand(B, -1, -1, -1), model.double())
    if not math.isfinite(float(ref)):
        assert not math.isfinite(l1), f"loss {l1} finite, reference {float(ref)}"
    for n in (0, 2):
        assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)), f"image {n}'s gradient depends on image 1"


def test_texture_step_and_range_loss_with_a_nan_texel(dev, ops, cow):
    """A NaN texel that a view samples makes the second approach's 'texture' loss non-finite; rgb_range_loss of a texture
    holding a NaN is non-finite, as torch.relu gives."""
    import losses as L
    import style_transfer as ST
    import utils as U
    from oracle import render_ref as RR
    from st3d.render import FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
    U.device = ST.device = L.device = dev
    S, T, B = 64, 64, 2
    tex_np = np.random.default_rng(0).random((T, T, 3), dtype=np.float32)
    gen = torch.Generator().manual_seed(0)
    elev, azim = RR.random_camera_angles(B, lambda k: torch.rand(k, generator=gen).numpy())
    R, Tt = RR.look_at_view_transform(2.10, elev, azim, at=(0, 0.10, 0.25))
    verts = torch.from_numpy(cow["verts"]).to(dev)
    faces = torch.from_numpy(cow["faces"].astype(np.int64)).to(dev)
    uvs = torch.from_numpy(cow["verts_uvs"])[None].to(dev)
    fuv = torch.from_numpy(cow["faces_uvs"].astype(np.int64))[None].to(dev)
    renderer = MeshRenderer(MeshRasterizer(None, RasterizationSettings(image_size=S)), SoftPhongShader())
    cams = FoVPerspectiveCameras(R=torch.from_numpy(R), T=torch.from_numpy(Tt), device=dev)
    vgg = U.get_vgg(seed=0)
    style = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(1)).to(dev)
    tex = torch.from_numpy(tex_np)[None].to(dev)
    with torch.no_grad():
        content, _ = U.render_meshes(renderer, U.build_mesh(uvs, fuv, tex, verts, faces), cams)

    def step(texture):
        out = U.setup_optimizations("texture", U.build_mesh(uvs, fuv, texture, verts, faces), 0.01)
        mesh = U.build_mesh(out["verts_uvs"], out["faces_uvs"], out["texture_map"], out["verts"], out["faces"])
        cur, _ = U.render_meshes(renderer, mesh, cams)
        loss = L.compute_second_approach_loss(cur, content, style.expand(B, -1, -1, -1), vgg, 1e6, 1.0, None, None, mesh,
                                              None, 'texture')
        out["optimizer"].zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), out["texture_map"].grad.detach(), mesh
    l0, gt0, mesh0 = step(tex)
    assert math.isfinite(l0) and float(L.rgb_range_loss(mesh0)) >= 0
    seen = gt0[0].abs().sum(-1)
    ty, tx = [int(i) for i in divmod(int(seen.argmax()), T)]
    assert float(seen[ty, tx]) > 0
    tb = tex.clone()
    tb[0, ty, tx, 1] = float("nan")
    l1, _, mesh1 = step(tb)
    assert not math.isfinite(l1), f"a NaN texel seen by a view gave the finite loss {l1}"
    assert not math.isfinite(float(L.rgb_range_loss(mesh1)))
