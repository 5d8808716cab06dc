"""fp64 restatement of the texture pyramid (csrc/texpyr.hip) in torch, independent of the library.

    sides(T, levels), offsets(sides), numel(T, levels)
    up2(c)          (n,n,3) -> (2n,2n,3): fine 2j = 0.25 c[j-1] + 0.75 c[j], fine 2j+1 = 0.75 c[j] + 0.25 c[j+1], clamped
    up2_t(g)        (2n,2n,3) -> (n,n,3): the adjoint written out as the gather (each coarse texel collects its <= 4x4 fine
                    footprint; a tap that does not exist is skipped and the clamped edge is folded into the edge weight)
    synth(params, T, L), adjoint(g, T, L), and the |.| companions the per-element error bounds are made of.

`mutant` switches on one deliberate mistake (tests/test_texpyr_ref.py checks that each is caught)."""
import torch

F64 = torch.float64


def sides(T, levels):
    if T < 1 or levels < 0:
        raise ValueError((T, levels))
    if levels == 0:
        out = [T]
        while out[-1] % 2 == 0 and out[-1] // 2 >= 4:
            out.append(out[-1] // 2)
        return out
    if levels > 1 and (T % (1 << (levels - 1)) or T >> (levels - 1) < 2):
        raise ValueError((T, levels))
    return [T >> l for l in range(levels)]


def offsets(sd):
    out = [0]
    for n in sd:
        out.append(out[-1] + 3 * n * n)
    return out


def numel(T, levels):
    return offsets(sides(T, levels))[-1]


def _taps(n, mutant=None):
    """For the 2n fine indices: (index a, index b, weight a, weight b) with c[a] * wa + c[b] * wb."""
    i = torch.arange(2 * n)
    j = i // 2
    odd = (i % 2 == 1)
    if mutant == "swap_odd_even":
        odd = ~odd
    a = torch.where(odd, j, j - 1)
    b = torch.where(odd, j + 1, j)
    wa = torch.where(odd, 0.75, 0.25).to(F64)
    wb = 1.0 - wa
    if mutant == "no_clamp":            # wrap instead of clamping
        a, b = a % n, b % n
    else:
        a, b = a.clamp(0, n - 1), b.clamp(0, n - 1)
    return a, b, wa, wb


def up2(c, mutant=None):
    n = c.shape[0]
    a, b, wa, wb = _taps(n, mutant)
    rows = wa[:, None, None] * c[a] + wb[:, None, None] * c[b]                     # y
    return wa[None, :, None] * rows[:, a] + wb[None, :, None] * rows[:, b]         # x


def _gather_1d(g, axis, mutant=None):
    """One axis of up2^T: coarse j <- 0.25 f[2j-1] + 0.75 f[2j] + 0.75 f[2j+1] + 0.25 f[2j+2], taps outside [0, 2n) skipped,
    the two edge texels with weight 1 on their nearest fine index."""
    g = g.movedim(axis, 0)
    n = g.shape[0] // 2
    out = torch.zeros((n,) + tuple(g.shape[1:]), dtype=g.dtype)
    j = torch.arange(n)
    base = (0.75, 0.25, 0.25, 0.75) if mutant == "swap_odd_even" else (0.25, 0.75, 0.75, 0.25)
    for t, w in enumerate(base):
        f = 2 * j - 1 + t
        ok = (f >= 0) & (f < 2 * n)
        wt = torch.full((n,), w, dtype=F64)
        if mutant != "no_clamp":
            if t == 1:
                wt[0] = 1.0
            if t == 2:
                wt[n - 1] = 1.0
        shape = (-1,) + (1,) * (g.dim() - 1)
        out[ok] = out[ok] + wt[ok].view(shape) * g[f[ok]]
    return out.movedim(0, axis)


def up2_t(g, mutant=None):
    return _gather_1d(_gather_1d(g, 1, mutant), 0, mutant)


def level(params, sd, l, mutant=None):
    off = offsets(sd)
    lo = off[l]
    if mutant == "offset_off_by_one_block" and l >= 2:
        lo = off[l - 1]
    n = sd[l]
    return params[lo:lo + 3 * n * n].view(n, n, 3)


def synth(params, T, levels, mutant=None):
    """-> (texture (T,T,3), [max |acc_l| for every level]) in the dtype of params (fp64 in the tests)."""
    sd = sides(T, levels)
    acc = level(params, sd, len(sd) - 1, mutant)
    amax = [float(acc.abs().max())]
    for l in range(len(sd) - 2, -1, -1):
        acc = level(params, sd, l, mutant) + up2(acc, mutant)
        amax.insert(0, float(acc.abs().max()))
    return acc, amax


def adjoint(g, T, levels, mutant=None):
    """g (T,T,3) -> flat gradient of params."""
    sd = sides(T, levels)
    out = [g.reshape(-1)]
    for _ in sd[1:]:
        g = up2_t(g, mutant)
        out.append(g.reshape(-1))
    if mutant == "offset_off_by_one_block" and len(out) > 2:
        out[1], out[2] = out[2], out[1]
    return torch.cat(out)


def adjoint_abs(g, T, levels):
    """M_l = (|up2|^T)^l |g| per element, laid out like the parameters: the scale of the backward's error bound."""
    return adjoint(g.abs(), T, levels)


def sign_step_coverage(grad_texture, T, levels):
    """One sign step on every level (Adam's first step moves an element by lr * sign(gradient)): the share of the T*T
    texels of the SYNTHESISED map that change."""
    gp = adjoint(grad_texture.to(F64), T, levels)
    delta, _ = synth(-torch.sign(gp), T, levels)
    return float((delta != 0).any(dim=2).double().mean())
