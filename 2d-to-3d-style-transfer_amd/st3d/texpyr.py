"""The texture as a pyramid of maps (Mordvintsev et al., "Differentiable Image Parameterizations", 2018).

The render backward reaches the texture only through the bilinear scatter of the shade kernel: a texel that no rendered
pixel's 2x2 footprint touches never gets a gradient, Adam never moves it, and the stylised map comes out speckled with
texels of the original (the reference's notes.txt:12-18).  Here the texture is the SUM of L maps of sides T, T/2, ...,
each upsampled bilinearly to T x T: a coarse texel collects the gradient of every fine texel under it and moves all of them.

    pyr = TexturePyramid(texture_map, levels)      # levels: 0 = auto, 1 = the plain map, L >= 2
    tex = pyr.texture()                            # (1,T,T,3), differentiable w.r.t. pyr.params
    Adam([pyr.params], lr)                         # ONE flat leaf: one Adam launch, one gradient, one checkpoint entry

Level 0 starts as the given map and every other level as +0.0, so the first texture() equals the map bit for bit.  Adam
normalises per element, so every level moves by about lr per step and their sum by up to L * lr: a pyramid run moves the
texture faster than a plain one at the same --lr (per-level step sizes are not implemented).
"""
import torch

from . import ops


class _Synth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, T, L):
        ctx.shape = (T, L)
        return ops.texpyr_synth(params.detach(), T, L)

    @staticmethod
    def backward(ctx, grad_texture):
        T, L = ctx.shape
        return ops.texpyr_adjoint(grad_texture.contiguous(), T, L), None, None


class TexturePyramid:
    def __init__(self, texture_map, levels=0):
        tex = texture_map.detach()
        if tex.dim() == 3:
            tex = tex[None]
        if tex.dim() != 4 or tex.shape[0] != 1 or tex.shape[3] != 3:
            raise ValueError(f"texture_map must be (1,T,T,3) or (T,T,3), got {tuple(texture_map.shape)}")
        if tex.shape[1] != tex.shape[2]:
            raise NotImplementedError("square texture maps only (the reference resizes to size x size)")
        self.side = int(tex.shape[1])
        self.sides = ops.texpyr_sides(self.side, levels)          # ValueError before anything is launched
        self.levels = len(self.sides)
        self.offsets = [3 * sum(n * n for n in self.sides[:l]) for l in range(self.levels + 1)]
        params = torch.zeros(self.offsets[-1], dtype=torch.float32, device=tex.device)
        params[:self.offsets[1]] = tex.to(torch.float32).reshape(-1)
        self.params = params.requires_grad_(True)

    def texture(self):
        """(1,T,T,3): the synthesised map, with the adjoint as its backward."""
        return _Synth.apply(self.params, self.side, self.levels)

    def level(self, l):
        """(T_l, T_l, 3) view of level l inside `params`."""
        if not 0 <= l < self.levels:
            raise IndexError(f"level {l} of a {self.levels}-level pyramid")
        n = self.sides[l]
        return self.params.detach()[self.offsets[l]:self.offsets[l + 1]].view(n, n, 3)

    def load_params(self, t):
        """Overwrite the parameters in place (checkpoint resume): the leaf and Adam's moments keep their identity."""
        if t.numel() != self.params.numel() or t.dim() != 1:
            raise ValueError(f"pyramid of sides {self.sides} holds {self.params.numel()} parameters in one flat tensor, "
                             f"got {tuple(t.shape)}")
        with torch.no_grad():
            self.params.copy_(t)
