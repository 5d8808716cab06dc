"""``first_approach.py`` of the reference (stylise each batch of views in 2-D, then fit the texture /
mesh to the stylised images through the renderer) on MI355X: same flags, defaults and artefacts
(``log.txt`` with ``Batch i, Step s, Loss x`` lines, ``2d_style_transfer/view_k.png``,
``final_render/``, ``final.obj``; reference first_approach.py:22-45, 147-225).

Phase A (reference :178-179) is ``style_transfer()``: fused VGG forward / loss / backward and a fused
Adam on the pixels.  Phase B (reference :191-217) is raster + fused shade + masked MSE + texture scatter
+ fused Adam: five HIP launches per step, no VGG.  Under ``python -m torch.distributed.run ...`` each
rank stylises and renders its slice of the batch's views and the phase-B gradient is summed inside
``optimizer.step()``.
"""
import torch
from tqdm import tqdm

from style_transfer import *  # noqa: F401,F403
from utils import *  # noqa: F401,F403
from losses import *  # noqa: F401,F403

from st3d.cli import BAKE_FLAGS, Flag, Run, make_parser

FLAGS = [
    Flag("n_mse_steps", int, 100, "phase-B steps (fit the 3-D parameters to the stylised views) per batch"),
    Flag("n_style_transfer_steps", int, 3000, "phase-A steps (2-D style transfer on the pixels) per batch"),
    Flag("output_path", str, "/content/output_first", "folder for log.txt, renders and the final mesh"),
    Flag("style_transfer_init", str, 'content', "what the 2-D style transfer starts from", ['noise', 'current', 'content']),
    Flag("style_transfer_lr", float, 0.01, "Adam step size of phase A"),
    Flag("mse_lr", float, 0.01, "Adam step size of phase B"),
] + BAKE_FLAGS              # --bake_texture: a closed-form start of phase B


def build_parser():
    return make_parser(FLAGS)


def _phase_a_start(run, args, content, outline, cams, style):
    """Initial pixels of the 2-D style transfer (reference :167-175) and the coverage of the render they come from
    (--style_mask object; for 'noise' the object is where the content render has it)."""
    if args.style_transfer_init == 'content':
        return content, outline
    if args.style_transfer_init == 'noise':
        return torch.rand(content.shape, device=run.device), outline
    img, cov = render_meshes(run.renderer, run.current_mesh(), cams)          # 'current'
    return apply_background(img, cov, background_type=args.current_background, background=style), cov


def main(argv=None):
    args = build_parser().parse_args(argv)
    run = Run(args, lr=args.mse_lr, image_dir="2d_style_transfer")
    mesh = run.opt['optimizable_mesh']

    run.say("Starting optimization...")
    for vb in run.batches():
        if vb.index < run.progress:         # --resume: these view batches were fitted before the checkpoint
            continue
        run.say(f"\nBatch {vb.index}")
        n_local = vb.hi - vb.lo
        targets = cams = outline = None
        if n_local:
            cams = run.cameras[vb.lo:vb.hi]
            style = run.style_image.expand(n_local, -1, -1, -1)
            with torch.no_grad():
                img, outline = render_meshes(run.renderer, run.content_mesh, cams)    # outline: --silhouette_weight's target
                content = apply_background(img, outline, background_type=args.content_background, background=style)
                start, region = _phase_a_start(run, args, content, outline, cams, style)
            # phase A: the whole batch is stylised at once; the result may leave [0,1], hence the clamp
            targets = finalize_tensor(style_transfer(start, content, style, run.vgg, steps=args.n_style_transfer_steps,
                                                     style_weight=args.style_weight, content_weight=args.content_weight,
                                                     lr=args.style_transfer_lr,
                                                     style_masks=region if args.style_mask == 'object' else None,
                                                     nnfm_weight=args.nnfm_weight, nnfm_layers=args.nnfm_layers,
                                                     swd_weight=args.swd_weight, swd_layers=args.swd_layers,
                                                     swd_directions=args.swd_directions,
                                                     swd_seed=args.seed if args.seed is not None else 0,
                                                     style_scales=run.style_scales,
                                                     style_scale_weights=run.style_scale_weights,
                                                     color=run.style_color,       # --preserve_color luminance
                                                     lap_weight=args.lap_weight, lap_pools=args.lap_pools))
            run.save_views(targets, vb.lo)
            run.bake_targets(targets, cams, f"batch {vb.index}")      # --bake_texture, off by default

        # phase B: masked MSE between the renders and the stylised views
        shown = 0
        for step in tqdm(range(args.n_mse_steps), desc="Optimizing", postfix=shown, disable=not run.main):
            run.optimizer.zero_grad()
            if n_local:
                mesh = run.current_mesh()
                rendered, cov = render_meshes(run.renderer, mesh, cams)
                loss = compute_first_approach_loss(rendered=rendered, masks=cov, target_rendered=targets,
                                                   verts=run.opt['verts'], target_verts=run.original_verts, mesh=mesh,
                                                   weights=run.loss_weights, opt_type=args.optimization_target,
                                                   batch_denom=vb.size)     # image term -> share of the batch mean
                # the masked MSE is masked by the CURRENT render's coverage and cannot see the outline move; this term can
                outline_term = run.silhouette_term(mesh, cams, outline, vb.size)
                if torch.is_tensor(outline_term):
                    loss = loss + outline_term
                anchor_term = run.chamfer_term(mesh)    # --chamfer_weight, off by default
                if torch.is_tensor(anchor_term):
                    loss = loss + anchor_term
                loss.backward()
            else:
                loss = run.idle_contribution()
            run.optimizer.step()
            shown = run.global_sum(loss).item()
            run.log(f'Batch {vb.index}, Step {step}, Loss {shown}')
        run.maybe_checkpoint(vb.index + 1)

    run.export(run.current_mesh())      # rebuilt from the parameters as the last step left them


if __name__ == "__main__":
    main()
