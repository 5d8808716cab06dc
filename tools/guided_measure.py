#!/usr/bin/env python3
"""Guided style loss, the GPU figures of DESIGN.md section 7 (profiles/guided_measure.json): config-2 steps (cow, 512^2, 8
views, texture-only) through the public API with style masks (`--style_mask object`) against none -- step time in
alternating windows of 30 steps, the weighted kernels' device times next to their unweighted twins (median, min, max of 20),
and the outcomes of 200 steps on white and noise backgrounds.

    python tools/guided_measure.py            # one MI355X; writes $OUT/guided_measure.json (default out/)

profiles/guided_bench_ab.jsonl is `python bench.py --gpus 1 --steps 100 --warmup 10` run alternately from a checkout of the
parent commit and from this tree, three times each, one JSON line per run."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-to-3d-style-transfer_amd")]
import numpy as np, torch
import _scenes as SC
import losses as L, style_transfer as ST, utils as U
from st3d import ops
from st3d.render import FoVPerspectiveCameras, MeshRasterizer, MeshRenderer, RasterizationSettings, SoftPhongShader
dev = torch.device("cuda:0")
U.device = ST.device = L.device = dev
S, B = 512, 8
out_json = {}
a = SC.load_asset("cow")
tex0 = SC.texture_at(a, S)
R, T = SC.random_cameras(B, seed=0)
vgg = U.get_vgg(seed=0)
style = SC.style_at(1, S).to(dev).expand(B, -1, -1, -1)


def ev_time(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record(); fn(); b_.record(); torch.cuda.synchronize()
        ts.append(a_.elapsed_time(b_))
    ts.sort()
    return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]        # median, min, max (ms)


class Scene:
    def __init__(self, bg):
        self.bg = bg
        self.mesh0, self.renderer, self.cams = SC.device_scene(U, dev, a["verts"], a["faces"], a["verts_uvs"], a["faces_uvs"], tex0, R, T, S)
        self.out = U.setup_optimizations("texture", self.mesh0, 0.01)
        with torch.no_grad():
            img, cov = U.render_meshes(self.renderer, self.mesh0, self.cams)
            self.content = U.apply_background(img, cov, background_type=bg, background=style)

    def step(self, guided):
        o = self.out
        mesh = U.build_mesh(o["verts_uvs"], o["faces_uvs"], o["texture_map"], o["verts"], o["faces"])
        img, cov = U.render_meshes(self.renderer, mesh, self.cams)
        cur = U.apply_background(img, cov, background_type=self.bg, background=style)
        loss = L.compute_perceptual_loss(cur, self.content, style, vgg, style_masks=cov if guided else None)
        o["optimizer"].zero_grad()
        loss.backward()
        o["optimizer"].step()
        return loss

    def evaluate(self):
        """loss triples of the current renders, unguided and guided"""
        o = self.out
        with torch.no_grad():
            mesh = U.build_mesh(o["verts_uvs"], o["faces_uvs"], o["texture_map"], o["verts"], o["faces"])
            img, cov = U.render_meshes(self.renderer, mesh, self.cams)
            cur = U.apply_background(img, cov, background_type=self.bg, background=style)
        plan = vgg.plan(B, S)
        plan.set_content(self.content); plan.set_style(style, B)
        plain = plan.loss(cur, 1e6, 1.0, want_grad=False)[0].cpu().tolist()
        guided = plan.loss(cur, 1e6, 1.0, want_grad=False, style_mask=cov)[0].cpu().tolist()
        plan.set_style_guidance(None)
        d = (o["texture_map"].detach().cpu() - torch.from_numpy(tex0)[None]).abs()
        return {"unguided_total_content_style": plain, "guided_total_content_style": guided,
                "texture_mean_abs_diff": float(d.mean()), "texture_max_abs_diff": float(d.max()),
                "texture_out_of_range_frac": float(((o["texture_map"] < 0) | (o["texture_map"] > 1)).float().mean())}


# ---- 1. step time, alternating windows of 30 steps
sc = {g: Scene("white") for g in (False, True)}
for g in (False, True):
    for _ in range(10):
        sc[g].step(g)
torch.cuda.synchronize()
windows = {False: [], True: []}
for w in range(4):
    for g in (False, True):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(30):
            sc[g].step(g)
        torch.cuda.synchronize()
        windows[g].append(round((time.perf_counter() - t0) / 30 * 1e3, 4))
out_json["step_ms_windows"] = {"none": windows[False], "object": windows[True]}
print("step ms  none", windows[False], " object", windows[True], flush=True)
del sc

# ---- 2. kernels: weighted against unweighted on the plan's shapes (B = 8 at 512^2)
mask = None
s0 = Scene("white")
with torch.no_grad():
    img, cov = U.render_meshes(s0.renderer, s0.mesh0, s0.cams)
planes, _ = ops.guidance_build(cov)
out_json["guidance_build_ms"] = ev_time(lambda: ops.guidance_build(cov))
C = (64, 128, 256, 512, 512)
gen = torch.Generator().manual_seed(0)
feats = [torch.rand(B, c, S >> l, S >> l, generator=gen).to(dev) for l, c in enumerate(C)]
out_json["gram_fwd_multi_ms"] = {"plain": ev_time(lambda: ops.gram_fwd_multi(feats)), "weighted": ev_time(lambda: ops.gram_fwd_multi(feats, qs=planes))}
kb = {}
for l in (1, 2, 3, 4):
    D = torch.randn(B, C[l], C[l], generator=gen); D = (D + D.transpose(1, 2)).to(dev).contiguous()
    outb = torch.zeros_like(feats[l])
    kb[f"tap{l}_C{C[l]}"] = {"plain": ev_time(lambda: ops.gram_bwd(D, feats[l], 1e-3, out=outb, gated=True)),
                            "weighted": ev_time(lambda: ops.gram_bwd(D, feats[l], 1e-3, out=outb, gated=True, q=planes[l]))}
out_json["gram_bwd_gated_accumulate_ms"] = kb
from oracle import perceptual_ref as P
w = P.make_vgg19_features(seed=0)._modules["0"].weight.detach()
_, wd = ops.conv3x3_pack(w.to(dev))
D0 = torch.randn(B, 64, 64, generator=gen); D0 = (D0 + D0.transpose(1, 2)).to(dev).contiguous()
gy = torch.randn(feats[0].shape, generator=gen).to(dev)
w0 = (planes[0] * planes[0]).contiguous()
need = (cov[:, 0] > 0).to(torch.uint8).contiguous()
seg, _ = ops.need_build(need, 1)
out_json["conv1_bwd_ms"] = {"plain": ev_time(lambda: ops.conv1_bwd(gy, feats[0], D0, 1e-3, wd)),
                            "weighted": ev_time(lambda: ops.conv1_bwd_weighted(gy, feats[0], D0, 1e-3, wd, w0)),
                            "plain_need": ev_time(lambda: ops.conv1_bwd_masked(gy, feats[0], D0, 1e-3, wd, seg, need)),
                            "weighted_need": ev_time(lambda: ops.conv1_bwd_weighted(gy, feats[0], D0, 1e-3, wd, w0, seg, need))}
print(json.dumps({k: out_json[k] for k in ("guidance_build_ms", "gram_fwd_multi_ms", "gram_bwd_gated_accumulate_ms", "conv1_bwd_ms")}), flush=True)
del feats, gy, s0

# ---- 3. 200 steps, white and noise, guided against not
res = {}
for bg in ("white", "noise"):
    for g in (False, True):
        torch.manual_seed(0)
        s = Scene(bg)
        first = None
        for i in range(200):
            l = s.step(g)
            if i == 0:
                first = float(l.detach())
        r = s.evaluate()
        r["first_loss"], r["last_loss"] = first, float(l.detach())
        res[f"{bg}_{'object' if g else 'none'}"] = r
        print(bg, "object" if g else "none", json.dumps(r), flush=True)
        del s
out_json["steps200"] = res
OUT = os.environ.get("OUT", os.path.join(ROOT, "out"))
os.makedirs(OUT, exist_ok=True)
json.dump(out_json, open(os.path.join(OUT, "guided_measure.json"), "w"), indent=1)
print("done")
