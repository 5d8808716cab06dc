"""Shared scaffolding of the two command-line drivers (first_approach.py / second_approach.py).

The reference repeats set-up, batching, logging and export in both scripts (first_approach.py:47-147,
219-225; second_approach.py:44-140,196-202).  Here that is one ``Run`` object: flag tables, device /
rank set-up, scene + renderer + VGG + cameras + optimiser, the view-batch schedule with its per-rank
slice, the log file and the final export.  The scripts keep only their loop bodies.
"""
import argparse
import math
import os
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import io as st3d_io
from . import optim as st3d_optim
from .render import (AmbientLights, DirectionalLights, FoVPerspectiveCameras, HeadLights, Materials, MeshRasterizer,
                     MeshRenderer, PointLights, RasterizationSettings, SoftPhongShader)

Flag = namedtuple("Flag", "name type default help choices nargs", defaults=(None, None))

_BACKGROUNDS = ['noise', 'style', 'white']
_TARGETS = ['texture', 'mesh', 'both']
_LIGHTS = ['ambient', 'point', 'directional', 'headlight']
_STYLE_MASKS = ['none', 'object']
_TEXTURE_TYPES = ['uv', 'vertex']
_LAPLACIANS = ['uniform', 'cot', 'cotcurv']
_VIEW_SELECTIONS = ['random', 'coverage']
_FILL_MODES = ['off', 'chart', 'map']
_COLOR_MODES = ['off', 'match', 'luminance']       # st3d.color.MODES
VIEW_CANDIDATES_DEFAULT, VIEW_CANDIDATES_MAX = 256, 4096        # (st3d.cover.MAX_CANDIDATES)
_NNFM_LAYERS = ['conv2_1', 'conv3_1', 'conv4_1', 'conv4_2', 'conv5_1']       # style_transfer.NNFM_LAYERS
_SWD_LAYERS = ['conv1_1', 'conv2_1', 'conv3_1', 'conv4_1', 'conv4_2', 'conv5_1']       # style_transfer.SWD_LAYERS


def nnfm_layers(text):
    """--nnfm_layers: a comma list of distinct names from conv2_1,conv3_1,conv4_1,conv4_2,conv5_1 -> the tuple"""
    names = tuple(s.strip() for s in text.split(','))
    if not names or len(set(names)) != len(names) or any(n not in _NNFM_LAYERS for n in names):
        raise argparse.ArgumentTypeError(f"expected a comma list of distinct names from {','.join(_NNFM_LAYERS)}, got {text!r}")
    return names


def swd_layers(text):
    """--swd_layers: a comma list of distinct names from conv1_1,conv2_1,conv3_1,conv4_1,conv4_2,conv5_1 -> the tuple"""
    names = tuple(s.strip() for s in text.split(','))
    if not names or len(set(names)) != len(names) or any(n not in _SWD_LAYERS for n in names):
        raise argparse.ArgumentTypeError(f"expected a comma list of distinct names from {','.join(_SWD_LAYERS)}, got {text!r}")
    return names


_STYLE_SCALES = (1, 2, 4)       # st3d.imgpyr.FACTORS
_MIN_SCALE_SIDE = 32            # st3d.imgpyr.MIN_PLAN_SIDE


def style_scales(text):
    """--style_scales: a comma list of strictly increasing factors from 1,2,4 -> the tuple"""
    try:
        factors = tuple(int(s.strip()) for s in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a comma list of factors from 1,2,4, got {text!r}")
    if any(f not in _STYLE_SCALES for f in factors) or any(b <= a for a, b in zip(factors, factors[1:])):
        raise argparse.ArgumentTypeError(f"expected strictly increasing factors from 1,2,4, got {text!r}")
    return factors


def style_scale_weights(text):
    """--style_scale_weights: a comma list of finite weights >= 0 -> the tuple"""
    try:
        weights = tuple(float(s.strip()) for s in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a comma list of numbers, got {text!r}")
    if any(not (math.isfinite(w) and w >= 0.0) for w in weights):
        raise argparse.ArgumentTypeError(f"expected finite weights >= 0, got {text!r}")
    return weights


_LAP_POOLS = (1, 2, 4, 8, 16)       # st3d.lap.POOLS
LAP_POOLS_DEFAULT = (4,)


def lap_pools(text):
    """--lap_pools: a comma list of strictly increasing pool sides from 1,2,4,8,16 -> the tuple"""
    try:
        pools = tuple(int(s.strip()) for s in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a comma list of pool sides from 1,2,4,8,16, got {text!r}")
    if any(p not in _LAP_POOLS for p in pools) or any(b <= a for a, b in zip(pools, pools[1:])):
        raise argparse.ArgumentTypeError(f"expected strictly increasing pool sides from 1,2,4,8,16, got {text!r}")
    return pools


def style_regions(text):
    """--style_regions: 'material', an axis with cuts (x:0, y:-0.1,0.2) or a .npy file of one label per face -> the text,
    once st3d.regions.parse_spec takes it"""
    from . import regions as _regions
    try:
        _regions.parse_spec(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text


# second_approach.py's own flags (the first and third approach have no per-region loss): --style_regions and its two lists
REGION_FLAGS = [
    Flag("style_regions", style_regions, None, "one style image per region of the mesh (Gatys et al. 2017, spatial control): "
         "'material' = the OBJ's usemtl groups in order of first appearance; 'x:c[,c...]' / 'y:...' / 'z:...' = slabs of the "
         "loaded mesh cut along that axis at the face centroids (k strictly increasing cuts give k + 1 regions, a centroid "
         "above a cut goes up); a .npy file = one integer label 0...R-1 per face.  At most 8 regions; background pixels "
         "belong to none.  The style term is then the guided Gram loss of every region against its own image "
         "(--region_styles), from the fragments of each step's own render; --style_path keeps serving the 'style' "
         "backgrounds.  Not with --style_mask object, --style_scales other than 1, --nnfm_weight, --swd_weight, "
         "--preserve_color, --supersample > 1 or several ranks.  Unset = off"),
    Flag("region_styles", str, None, "with --style_regions: exactly one style image per region, region r takes the r-th path",
         None, '+'),
    Flag("region_style_weights", float, None, "with --style_regions: one finite weight >= 0 per region on its style term; "
         "default all 1", None, '+'),
]


def _check_region_args(args):
    """check_args for --style_regions / --region_styles / --region_style_weights -> None or the complaint"""
    spec = getattr(args, "style_regions", None)
    styles, weights = getattr(args, "region_styles", None), getattr(args, "region_style_weights", None)
    if spec is None:
        if styles is not None:
            return "--region_styles needs --style_regions: without regions there is nothing to give the images to"
        if weights is not None:
            return "--region_style_weights needs --style_regions: without regions there is nothing to weight"
        return None
    from . import regions as _regions
    if styles is None:
        return "--style_regions needs --region_styles: one style image per region"
    if len(styles) > _regions.MAX_REGIONS:
        return f"--region_styles names {len(styles)} images; there are at most {_regions.MAX_REGIONS} regions"
    if weights is not None:
        if any(not (math.isfinite(w) and w >= 0.0) for w in weights):
            return "--region_style_weights must be finite and >= 0"
        if len(weights) != len(styles):
            return (f"--region_style_weights must give one weight per region: got {len(weights)} for the {len(styles)} images "
                    "of --region_styles")
    parsed = _regions.parse_spec(spec)
    if parsed[0] == "axis" and len(parsed[2]) + 1 != len(styles):
        return (f"--style_regions {spec} makes {len(parsed[2]) + 1} regions but --region_styles names {len(styles)} images: "
                "exactly one per region")
    if getattr(args, "style_mask", "none") == 'object':
        return ("--style_regions cannot be combined with --style_mask object: the regions already exclude the background, "
                "and one region over every face is that mask")
    if tuple(getattr(args, "style_scales", None) or (1,)) != (1,) or getattr(args, "style_scale_weights", None) is not None:
        return ("--style_regions needs --style_scales 1: the region planes are built at the render's side only, the image "
                "pyramid has none")
    if getattr(args, "nnfm_weight", 0.0):
        return "--style_regions cannot be combined with --nnfm_weight: the NNFM term has no per-region style"
    if getattr(args, "swd_weight", 0.0):
        return "--style_regions cannot be combined with --swd_weight: the sliced Wasserstein term has no per-region style"
    if getattr(args, "preserve_color", "off") != "off":
        return ("--style_regions needs --preserve_color off: the colour matching prepares one style image, the regions have "
                "several")
    if getattr(args, "supersample", 1) > 1:
        return ("--style_regions needs --supersample 1: a supersampled pixel can see faces of several regions, the planes "
                "take one face per pixel")
    if parsed[0] == "material" and os.path.isfile(getattr(args, "obj_path", "")):
        groups = _regions.count_material_groups(args.obj_path)
        if groups < 2:
            return (f"--style_regions material needs an OBJ with at least 2 usemtl groups; {args.obj_path} has {groups}, so the "
                    "regions would be the whole object (--style_mask object does that)")
        if groups != len(styles):
            return (f"--style_regions material finds {groups} usemtl groups in {args.obj_path} but --region_styles names "
                    f"{len(styles)} images: exactly one per region")
    return None


def edge_target_length(text):
    """--edge_target_length: a length, or the literal 'mean' (the loaded mesh's mean edge length, resolved by Run)"""
    if text == 'mean':
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected a number or 'mean', got {text!r}")

# name, type, default and choices are the reference's (first_approach.py:23-45, second_approach.py:23-42); note
# `type=bool` flags keep argparse's "any non-empty string is True" behaviour of the reference.
SHARED_FLAGS = [
    Flag("n_views", int, 6, "how many camera views surround the object"),
    Flag("obj_path", str, "./objects/cow_mesh/cow.obj", "Wavefront OBJ to stylise"),
    Flag("style_path", str, "./imgs/Style_1.jpg", "style image"),
    Flag("style_weight", float, 1e6, "multiplier of the Gram (style) term"),
    Flag("content_weight", float, 1.0, "multiplier of the conv4_2 (content) term"),
    Flag("resize_texture", bool, True, "resample the texture map to size x size"),
    Flag("size", int, 768, "side of the rendered images in pixels"),
    Flag("batch_size", int, 4, "views per optimisation step"),
    Flag("content_background", str, 'white', "what fills the uncovered pixels of the content renders", _BACKGROUNDS),
    Flag("current_background", str, 'white', "what fills the uncovered pixels of the current renders", _BACKGROUNDS),
    Flag("randomize_views", bool, True, "random cameras on a sphere instead of the fixed turntable"),
    Flag("optimization_target", str, "texture", "which tensors Adam updates", _TARGETS),
    Flag("main_loss_weight", float, 3.0, "weight of the image term when the mesh is optimised"),
    Flag("mesh_edge_loss_weight", float, 1.0, "weight of the edge-length regulariser"),
    Flag("mesh_laplacian_smoothing_weight", float, 1.0, "weight of the uniform-Laplacian regulariser"),
    Flag("mesh_normal_consistency_weight", float, 1.0, "weight of the normal-consistency regulariser"),
    Flag("mesh_verts_weight", float, 1.0, "weight of the distance to the original vertices"),
    # additions; the defaults keep the reference behaviour
    Flag("vgg_weights", str, None, "local VGG-19 state_dict (never downloaded); default ST3D_VGG19_WEIGHTS or seeded weights"),
    Flag("seed", int, None, "seed for camera sampling / noise (the reference is unseeded)"),
    Flag("verts_lr", float, None, "separate Adam step size for the vertices when both are optimised (notes.txt:29 of the reference)"),
    Flag("checkpoint_every", int, 0, "write <output_path>/checkpoint.pt (parameters + Adam state) every N epochs/batches; 0 = never"),
    Flag("resume", str, None, "checkpoint.pt to continue from"),
    Flag("lights", str, "ambient", "shading of every render: white ambient (the reference's), a point or directional light "
         "(PyTorch3D's default colours), or a point light at each view's camera", _LIGHTS),
    Flag("light_xyz", float, [0.0, 1.0, 0.0], "location of the point light / direction towards the directional light", None, 3),
    Flag("shininess", float, 64.0, "Phong exponent of the material (lit runs)"),
    Flag("silhouette_weight", float, 0.0, "weight of the silhouette term that holds the outline of the content mesh when the "
         "vertices move (optimization_target mesh / both); 0 = off"),
    Flag("silhouette_sigma", float, 1e-4, "sigma of the soft silhouette (SoftSilhouetteShader's BlendParams.sigma)"),
    Flag("silhouette_faces_per_pixel", int, None, "faces per pixel of the silhouette term, 1..64, on the silhouette rasteriser "
         "(PyTorch3D's silhouette tutorial uses 50); unset = the general rasteriser at 8"),
    Flag("style_mask", str, 'none', "region the style term's Gram matrices are taken over: 'none' = the whole image (the "
         "reference's loss), 'object' = the coverage of each render being optimised (guided Gram matrices, Gatys et al. 2017), "
         "so that the background neither takes part in the style term nor draws its gradient", _STYLE_MASKS),
    Flag("texture_pyramid_levels", int, 1, "optimise the texture as the sum of N maps of halving sides, so that texels no "
         "rendered pixel touches move with their neighbours; 1 = the plain map, 0 = as many levels as the side allows "
         "(down to a side of 4..7).  Every level moves by about lr a step, their sum by up to N x lr"),
    Flag("supersample", int, 1, "rasterise and shade every render of the run (current, content, final) at N x size and hand the "
         "loss the N x N box-filtered image at size: each pixel then carries gradient to N^2 texture footprints and "
         "silhouette pixels get a fractional coverage; 1..4, N x size <= 4096, 1 = off"),
    Flag("texture_mip_levels", int, 1, "sample the texture of every render trilinearly from a mip chain of N levels at each "
         "pixel's own level of detail, so that a pixel over several texels reads and moves all of them; 1 = off (bilinear on "
         "the map itself), 0 = the full chain (down to a side of 2 or the first odd side).  White ambient light, "
         "--supersample 1 only"),
    Flag("texture_type", str, 'uv', "what carries the colour: 'uv' = the OBJ's UV atlas and texture map (the reference's "
         "TexturesUV), 'vertex' = one RGB triple per vertex interpolated over each face (PyTorch3D's TexturesVertex), for "
         "meshes without UVs; started from the map sampled at each vertex's UV when the OBJ has one, else from seeded grey "
         "noise.  White ambient light, --supersample 1, --texture_mip_levels 1, --texture_pyramid_levels 1, no --tv_weight",
         _TEXTURE_TYPES),
    Flag("texture_atlas", int, 0, "optimise a per-face texel atlas (PyTorch3D's TexturesAtlas) of N x N texels per face instead "
         "of a UV-mapped texture: no UV chart, no seams, F N^2 texels addressed by each fragment's barycentrics (nearest "
         "texel; --supersample is its anti-aliasing); 0 = off, 1...64.  Started from the map sampled at every texel's centre "
         "when the OBJ has UVs and a map, else from seeded grey noise.  --optimization_target texture, --texture_type uv, white "
         "ambient light, --texture_mip_levels 1, --texture_pyramid_levels 1, no --tv_weight"),
    Flag("laplacian_method", str, 'uniform', "Laplacian of the smoothing regulariser (PyTorch3D's mesh_laplacian_smoothing "
         "methods): 'uniform' = the plain mean of the neighbours (the reference's), 'cot' = cotangent weights, zero on a flat "
         "patch whatever its triangulation, 'cotcurv' = cotangent weights over the vertex's area (mean curvature).  "
         "--optimization_target mesh / both only", _LAPLACIANS),
    Flag("edge_target_length", edge_target_length, 0.0, "length the edge regulariser pulls every edge to: 0 = the reference's "
         "(edges can only shrink), 'mean' = the mean edge length of the loaded mesh, or a length >= 0.  "
         "--optimization_target mesh / both only"),
    Flag("chamfer_weight", float, 0.0, "weight of the Chamfer term that ties the moving surface to the loaded one: N points "
         "redrawn every step from the current mesh against N points sampled once from the loaded mesh (PyTorch3D's "
         "sample_points_from_meshes + chamfer_distance).  Unlike --mesh_verts_weight it leaves a vertex free to slide along "
         "the surface; at its optimum it is about 2 area / (pi N), not 0.  --optimization_target mesh / both only; 0 = off"),
    Flag("chamfer_samples", int, 5000, "points per cloud of the Chamfer term, 1...1048576"),
    Flag("nnfm_weight", float, 0.0, "weight of the nearest-neighbour feature matching style term (ARF, Zhang et al. 2022): every "
         "VGG feature vector of a render looks up its nearest style feature by cosine distance, the term is the mean distance.  "
         "Keeps the stroke-level detail the Gram term averages away; joins the Gram term, or replaces it with --style_weight 0.  "
         "--style_mask object restricts it to the object's coverage.  Costs its own partial VGG forward and backward per "
         "step; 0 = off"),
    Flag("nnfm_layers", nnfm_layers, ('conv3_1',), "taps of the NNFM term, a comma list from conv2_1,conv3_1,conv4_1,conv4_2,"
         "conv5_1; their terms are added"),
    Flag("swd_weight", float, 0.0, "weight of the sliced Wasserstein style term (Heitz et al. 2021): the VGG features of a render "
         "and of the style image are projected onto random directions, sorted, and matched quantile by quantile -- the whole "
         "feature distribution, not its second moments.  Joins the Gram term, or replaces it with --style_weight 0.  "
         "--style_mask object takes the distribution over the object's coverage only.  The directions are redrawn every step "
         "from a generator seeded with --seed (0 when unset).  Costs its own partial VGG forward and backward per step; 0 = off"),
    Flag("swd_layers", swd_layers, ('conv2_1', 'conv3_1', 'conv4_1', 'conv5_1'), "taps of the sliced Wasserstein term, a comma "
         "list from conv1_1,conv2_1,conv3_1,conv4_1,conv4_2,conv5_1; their terms are added"),
    Flag("swd_directions", int, 0, "directions each tap is projected onto, 1...512; 0 = as many as the tap has channels"),
    Flag("verts_diffusion", float, 0.0, "optimise the vertices through u = (I + lambda L) verts, L the combinatorial Laplacian of "
         "the mesh (Nicolet et al. 2021, 'Large Steps in Inverse Rendering of Geometry'): Adam steps on u with one denominator "
         "for the whole tensor, and every step solves for the vertices by conjugate gradients, so the surface moves coherently "
         "instead of vertex by vertex.  The value is lambda, finite and >= 0 (the paper's examples use about 19); --verts_lr "
         "is the step size of u.  --optimization_target mesh / both only; 0 = off"),
    Flag("texture_lod_bias", float, 0.0, "added to every pixel's level of detail before it is clamped to the chain "
         "(--texture_mip_levels): negative = sharper, positive = blurrier"),
    Flag("view_selection", str, 'random', "which cameras the run looks through: 'random' = n_views random directions (the "
         "reference's), 'coverage' = --view_candidates random directions are drawn instead and the n_views of them that "
         "together touch the most texels of the map are picked greedily, once, on the loaded mesh, so that fewer texels stay "
         "unseen for the whole run.  The selection always marks the plain bilinear footprint at --size, whatever --supersample "
         "or --texture_mip_levels say; it writes texel_coverage.png (how many of the picked views touch each texel, over "
         "n_views).  --texture_type uv without --texture_atlas only", _VIEW_SELECTIONS),
    Flag("view_candidates", int, VIEW_CANDIDATES_DEFAULT, "candidate directions --view_selection coverage picks from, n_views..."
         "4096"),
    Flag("fill_unseen", str, 'off', "at export, give every texel the run never moved (its bits are still the loaded map's) a "
         "colour interpolated from the texels it did move, by a pull-push fill of the map (st3d.fill): final_render/, final.obj "
         "and its PNG show the filled map, texel_filled.png which texels were filled.  'chart' writes only the texels of the "
         "chart and its 1.5-texel gutter (a square map only), 'map' every texel -- the dilation a mip-mapping viewer needs.  "
         "--optimization_target texture / both, --texture_type uv without --texture_atlas", _FILL_MODES),
    Flag("style_scales", style_scales, None, "evaluate the style and content terms on the renders and on copies of them reduced "
         "by these factors, a comma list of strictly increasing values from 1,2,4, and add the terms (an image pyramid: Gatys et "
         "al. 2017, Heitz et al. 2021): VGG's receptive fields are fixed in pixels, so the reduced copies are where the large "
         "shapes of the style image are seen.  --size must be divisible by the largest factor and leave a side >= 32.  Each "
         "factor f costs a VGG pass at side size / f; the NNFM and sliced Wasserstein terms stay at full resolution.  "
         "Default 1: the single-scale loss"),
    Flag("style_scale_weights", style_scale_weights, None, "one finite weight >= 0 per factor of --style_scales, a comma list; "
         "a weight of 0 leaves its scale out.  Default: all 1"),
    Flag("preserve_color", str, 'off', "keep the asset's own palette and take only the strokes of the style image (Gatys et al. "
         "2017, section 5): 'match' recolours the style image once, by an affine map, so that its pixel mean and covariance "
         "equal those of the loaded mesh seen through the run's cameras; 'luminance' shows every style and content term the "
         "luminance of render, content and style only, and at export puts the optimised luminance back under the loaded "
         "colours.  Both write style_matched.png.  --optimization_target texture / both", _COLOR_MODES),
    Flag("lap_weight", float, 0.0, "weight of the Laplacian content term (Li et al. 2017, 'Laplacian-Steered Neural Style "
         "Transfer'): the mean squared difference between the 5-point Laplacian of the average-pooled render and that of the "
         "average-pooled content render, per channel.  Keeps the fine detail of the asset (eyes, panel lines, print) that the "
         "conv4_2 content term does not see, when --nnfm_weight or --swd_weight pull hard.  The term is a mean over residuals "
         "of [0,1] images, so small weights do nothing: below about 1e3 it cannot matter next to --style_weight 1e6 (the useful "
         "range is not measured yet, DESIGN.md 7).  Needs --content_background "
         "equal to --current_background and neither 'noise'.  One fused pass per pool side and step; 0 = off"),
    Flag("lap_pools", lap_pools, LAP_POOLS_DEFAULT, "pool sides of the Laplacian content term, a comma list of strictly "
         "increasing values from 1,2,4,8,16; their terms are added.  --size must be divisible by each and leave a pooled side "
         ">= 2.  Needs --lap_weight"),
]

# the fitting phase of first_approach.py / third_approach.py only: each script adds them to its own table
_BAKE_MODES = ['off', 'mean', 'best']
BAKE_POWER_DEFAULT, BAKE_MIN_COS_DEFAULT = 2.0, 0.1
BAKE_FLAGS = [
    Flag("bake_texture", str, 'off', "before the fitting steps of a batch, bake the batch's stylised views into the texture map "
         "by UV-space back-projection (st3d.bake): every texel of the chart takes the colour the views show at its surface "
         "point, 'mean' = blended by the viewing angle, 'best' = from the squarest view alone.  A closed-form head start worth "
         "tens of fitting steps, with no optimiser state; --n_mse_steps 0 is then a pure bake.  The bake always reads the plain "
         "fragments at --size, whatever --supersample or --texture_mip_levels say.  --optimization_target texture / both, "
         "--texture_type uv without --texture_atlas, --texture_pyramid_levels 1, white ambient light, one process only",
         _BAKE_MODES),
    Flag("bake_power", float, BAKE_POWER_DEFAULT, "a view's weight in the bake is |cos of its viewing angle|^N, N >= 0"),
    Flag("bake_min_cos", float, BAKE_MIN_COS_DEFAULT, "the bake ignores a view that sees the texel's face at |cos| below this, "
         "0...1"),
]

# regularisers the reference defines but never switches on (losses.py:48-65, notes.txt:36,39); weight 0 = off
REGULARISER_FLAGS = [
    Flag("tv_weight", float, 0.0, "weight of the masked total-variation term on the current renders"),
    Flag("rgb_range_weight", float, 0.0, "weight of the out-of-[0,1] penalty on the texture map"),
    Flag("texture_l2_weight", float, 0.0, "weight of the squared distance to the original texture map"),
]


def check_args(args):
    """What the flags rule out together, found when they are read -- before any GPU work.  -> None or the complaint."""
    if getattr(args, "silhouette_weight", 0.0) and getattr(args, "optimization_target", None) == 'texture':
        return ("--silhouette_weight needs --optimization_target mesh or both: with 'texture' the vertices do not move and "
                "the term would be a constant")
    method, target = getattr(args, "laplacian_method", "uniform"), getattr(args, "edge_target_length", 0.0)
    if target != 'mean' and not (math.isfinite(target) and target >= 0.0):
        return "--edge_target_length must be 'mean' or a finite length >= 0"
    if (method != "uniform" or target != 0.0) and getattr(args, "optimization_target", None) == 'texture':
        return ("--laplacian_method / --edge_target_length need --optimization_target mesh or both: with 'texture' the vertices "
                "do not move and the mesh regularisers do not run")
    chamfer = getattr(args, "chamfer_weight", 0.0)
    if not (math.isfinite(chamfer) and chamfer >= 0.0):
        return "--chamfer_weight must be finite and >= 0"
    if chamfer and getattr(args, "optimization_target", None) == 'texture':
        return ("--chamfer_weight needs --optimization_target mesh or both: with 'texture' the vertices do not move and the "
                "term would be a constant")
    diffusion = getattr(args, "verts_diffusion", 0.0)
    if not (math.isfinite(diffusion) and diffusion >= 0.0):
        return "--verts_diffusion must be finite and >= 0"
    if diffusion and getattr(args, "optimization_target", None) == 'texture':
        return ("--verts_diffusion needs --optimization_target mesh or both: with 'texture' the vertices do not move and "
                "there is nothing to precondition")
    if not 1 <= getattr(args, "chamfer_samples", 5000) <= 1 << 20:
        return "--chamfer_samples must be in 1...1048576"
    nnfm = getattr(args, "nnfm_weight", 0.0)
    if not (math.isfinite(nnfm) and nnfm >= 0.0):
        return "--nnfm_weight must be finite and >= 0"
    swd = getattr(args, "swd_weight", 0.0)
    if not (math.isfinite(swd) and swd >= 0.0):
        return "--swd_weight must be finite and >= 0"
    if not 0 <= getattr(args, "swd_directions", 0) <= 512:
        return "--swd_directions must be 0 (the channels of each tap) or in 1...512"
    if not getattr(args, "silhouette_sigma", 1e-4) > 0.0:
        return "--silhouette_sigma must be positive"
    k = getattr(args, "silhouette_faces_per_pixel", None)
    if k is not None and not 1 <= k <= 64:
        return "--silhouette_faces_per_pixel must be in 1..64"
    levels = getattr(args, "texture_pyramid_levels", 1)
    if levels < 0:
        return "--texture_pyramid_levels must be 0 (auto), 1 (off) or the number of levels"
    if levels != 1 and getattr(args, "optimization_target", None) == 'mesh':
        return ("--texture_pyramid_levels needs --optimization_target texture or both: with 'mesh' the texture is not "
                "optimised")
    n = getattr(args, "supersample", 1)
    if not 1 <= n <= 4:
        return "--supersample must be in 1..4"
    if n * getattr(args, "size", 0) > 4096:
        return f"--supersample {n} x --size {args.size} exceeds the rasteriser's 4096 pixels a side"
    if n > 1 and getattr(args, "silhouette_weight", 0.0):
        return ("--supersample > 1 cannot be combined with --silhouette_weight: alpha-only (silhouette) renders are not "
                "supersampled")
    mip = getattr(args, "texture_mip_levels", 1)
    if not 0 <= mip <= 16:
        return "--texture_mip_levels must be 0 (full chain), 1 (off) or the number of levels, at most 16"
    bias = getattr(args, "texture_lod_bias", 0.0)
    if not math.isfinite(bias):
        return "--texture_lod_bias must be finite"
    if mip != 1:
        if n > 1:
            return "--texture_mip_levels cannot be combined with --supersample > 1: the supersampled kernels do not mip-map"
        if getattr(args, "lights", "ambient") != "ambient":
            return (f"--texture_mip_levels needs --lights ambient: the lit kernels do not mip-map (got --lights "
                    f"{args.lights})")
        size = getattr(args, "size", 0)
        if mip > 1 and getattr(args, "resize_texture", True) and (size % (1 << (mip - 1)) or size >> (mip - 1) < 2):
            return (f"--texture_mip_levels {mip} needs a texture side divisible by {1 << (mip - 1)} with a coarsest side >= 2; "
                    f"--resize_texture makes it --size = {size}")
    elif bias != 0.0:
        return "--texture_lod_bias needs --texture_mip_levels other than 1"
    if getattr(args, "texture_type", "uv") == "vertex":
        if levels != 1:
            return "--texture_type vertex needs --texture_pyramid_levels 1: per-vertex colours have no map to build a pyramid of"
        if mip != 1:
            return "--texture_type vertex needs --texture_mip_levels 1: per-vertex colours have no map to filter"
        if n > 1:
            return "--texture_type vertex needs --supersample 1: the supersampled kernels have no vertex-colour path"
        if getattr(args, "lights", "ambient") != "ambient":
            return (f"--texture_type vertex needs --lights ambient: the lit kernels have no vertex-colour path (got --lights "
                    f"{args.lights})")
        if getattr(args, "tv_weight", 0.0) > 0:
            return "--texture_type vertex cannot be combined with --tv_weight > 0: per-vertex colours lie on no grid"
    atlas = getattr(args, "texture_atlas", 0)
    if not 0 <= atlas <= 64:
        return "--texture_atlas must be 0 (off) or the texels per face side, 1...64"
    if atlas:
        if getattr(args, "texture_type", "uv") != "uv":
            return (f"--texture_atlas cannot be combined with --texture_type {args.texture_type}: the atlas takes the place of "
                    "the colour carrier")
        if levels != 1:
            return "--texture_atlas needs --texture_pyramid_levels 1: an atlas has no map to build a pyramid of"
        if mip != 1:
            return "--texture_atlas needs --texture_mip_levels 1: the atlas is sampled at its nearest texel and has no mip chain"
        if getattr(args, "lights", "ambient") != "ambient":
            return f"--texture_atlas needs --lights ambient: the lit kernels have no atlas path (got --lights {args.lights})"
        if getattr(args, "tv_weight", 0.0) > 0:
            return ("--texture_atlas cannot be combined with --tv_weight > 0: the term's gradient reaches an atlas through no "
                    "filter, texel by texel")
        target_ = getattr(args, "optimization_target", "texture")
        if target_ != "texture":
            return (f"--texture_atlas needs --optimization_target texture: the nearest-texel colour moves no vertex (got "
                    f"--optimization_target {target_})")
    candidates = getattr(args, "view_candidates", VIEW_CANDIDATES_DEFAULT)
    if getattr(args, "view_selection", "random") == "coverage":
        if getattr(args, "texture_type", "uv") == "vertex":
            return "--view_selection coverage needs --texture_type uv: per-vertex colours have no texels to cover"
        if atlas:
            return "--view_selection coverage needs --texture_atlas 0: the selection covers the texels of a UV-mapped texture"
        if not getattr(args, "n_views", 1) <= candidates <= VIEW_CANDIDATES_MAX:
            return (f"--view_candidates must be in n_views...{VIEW_CANDIDATES_MAX} (got {candidates} with --n_views "
                    f"{getattr(args, 'n_views', 1)})")
    elif candidates != VIEW_CANDIDATES_DEFAULT:
        return "--view_candidates needs --view_selection coverage"
    power = getattr(args, "bake_power", BAKE_POWER_DEFAULT)
    if not (math.isfinite(power) and power >= 0.0):
        return "--bake_power must be finite and >= 0"
    min_cos = getattr(args, "bake_min_cos", BAKE_MIN_COS_DEFAULT)
    if not 0.0 <= min_cos <= 1.0:
        return "--bake_min_cos must be in 0...1"
    if getattr(args, "bake_texture", "off") != "off":
        if getattr(args, "optimization_target", "texture") == 'mesh':
            return ("--bake_texture needs --optimization_target texture or both: with 'mesh' the texture is not optimised and "
                    "there is no map to bake into")
        if getattr(args, "texture_type", "uv") == "vertex":
            return "--bake_texture needs --texture_type uv: per-vertex colours have no texels to bake into"
        if atlas:
            return "--bake_texture needs --texture_atlas 0: the bake walks the texels of a UV-mapped texture"
        if levels != 1:
            return ("--bake_texture needs --texture_pyramid_levels 1: the bake writes the plain map, a pyramid's levels are not "
                    "solved for")
        if getattr(args, "lights", "ambient") != "ambient":
            return (f"--bake_texture needs --lights ambient: a lit image would bake the lighting into the albedo (got --lights "
                    f"{args.lights})")
    elif power != BAKE_POWER_DEFAULT or min_cos != BAKE_MIN_COS_DEFAULT:
        return "--bake_power / --bake_min_cos need --bake_texture mean or best"
    if getattr(args, "fill_unseen", "off") != "off":
        if getattr(args, "optimization_target", "texture") == 'mesh':
            return ("--fill_unseen needs --optimization_target texture or both: with 'mesh' no texel is optimised and there is "
                    "nothing to fill from")
        if getattr(args, "texture_type", "uv") == "vertex":
            return "--fill_unseen needs --texture_type uv: per-vertex colours have no texels to fill"
        if atlas:
            return "--fill_unseen needs --texture_atlas 0: the fill walks the texels of a UV-mapped texture"
    if getattr(args, "preserve_color", "off") != "off" and getattr(args, "optimization_target", "texture") == 'mesh':
        return ("--preserve_color needs --optimization_target texture or both: with 'mesh' no colour is optimised and there is "
                "nothing to preserve")
    scales, scale_weights = getattr(args, "style_scales", None), getattr(args, "style_scale_weights", None)
    if scales is None:
        if scale_weights is not None:
            return "--style_scale_weights needs --style_scales"
    else:
        if scale_weights is not None and len(scale_weights) != len(scales):
            return f"--style_scale_weights must give one weight per factor of --style_scales ({len(scales)}), got {len(scale_weights)}"
        size = getattr(args, "size", 0)
        if scales != (1,) and (size % scales[-1] or size // scales[-1] < _MIN_SCALE_SIDE):
            return (f"--style_scales {','.join(str(f) for f in scales)} needs --size divisible by {scales[-1]} with --size / "
                    f"{scales[-1]} >= {_MIN_SCALE_SIDE}, got --size {size}")
    complaint = _check_lap_args(args)
    if complaint:
        return complaint
    return _check_region_args(args)


def _check_lap_args(args):
    """--lap_weight / --lap_pools against each other, --size and the backgrounds -> None or the complaint"""
    lap = getattr(args, "lap_weight", 0.0)
    if not (math.isfinite(lap) and lap >= 0.0):
        return "--lap_weight must be finite and >= 0"
    pools = tuple(getattr(args, "lap_pools", None) or LAP_POOLS_DEFAULT)
    if not lap:
        if pools != LAP_POOLS_DEFAULT:
            return "--lap_pools needs --lap_weight"
        return None
    size = getattr(args, "size", 0)
    for p in pools:
        if size % p or size // p < 2:
            return (f"--lap_pools {','.join(str(q) for q in pools)} needs --size divisible by {p} with --size / {p} >= 2, got "
                    f"--size {size}")
    content_bg, current_bg = getattr(args, "content_background", "white"), getattr(args, "current_background", "white")
    if content_bg != current_bg or 'noise' in (content_bg, current_bg):
        return (f"--lap_weight needs --content_background equal to --current_background and neither 'noise' (got {content_bg} "
                f"and {current_bg}): the term compares whole images, and differing backgrounds would be counted as lost content")
    return None


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        parsed = super().parse_args(args, namespace)
        complaint = check_args(parsed)
        if complaint:
            self.error(complaint)
        if getattr(parsed, "style_scales", (1,)) is None:       # unset: the single-scale loss
            parsed.style_scales = (1,)
        return parsed


def make_parser(extra_flags):
    parser = _Parser()
    for fl in list(extra_flags) + SHARED_FLAGS:
        kw = {"type": fl.type, "default": fl.default, "help": fl.help}
        if fl.choices:
            kw["choices"] = fl.choices
        if fl.nargs:
            kw["nargs"] = fl.nargs
        parser.add_argument("--" + fl.name, **kw)
    return parser


def make_lights(args, device):
    """--lights / --light_xyz / --shininess -> (lights, materials) of every render of the run (current and content
    renders, final_render/).  'ambient' is the reference's white AmbientLights, rendered exactly as before."""
    kind = getattr(args, "lights", "ambient")
    if kind == "ambient":
        return AmbientLights(device=device), None
    materials = Materials(shininess=float(args.shininess), device=device)
    xyz = (tuple(float(x) for x in args.light_xyz),)
    if kind == "point":
        return PointLights(location=xyz, device=device), materials
    if kind == "directional":
        return DirectionalLights(direction=xyz, device=device), materials
    if kind == "headlight":
        return HeadLights(device=device), materials
    raise ValueError(f"unknown --lights {kind!r}")


def load_scene(obj_path, size, resize_texture, device):
    """OBJ + its texture -> (verts (V,3), faces (F,3), verts_uvs (1,VT,2), faces_uvs (1,F,3), map (1,T,T,3)) on
    `device`, the map resampled to size x size when asked (reference second_approach.py:77-97)."""
    verts, faces, aux = st3d_io.load_obj(obj_path)
    if aux.verts_uvs is None or faces.textures_idx is None or not aux.texture_images:
        # e.g. objects/teapot_mesh/teapot.obj (faces `v//vn`, no mtllib): the reference crashes at
        # first_approach.py:85-88, so there is no behaviour to match.  Per-vertex spherical UVs
        # and a mid-grey texture with seeded noise are synthesised so BASELINE config 4 can run.
        print(f"WARNING: {obj_path} has no UVs / texture; synthesising spherical UVs and a grey noise texture")
        uvs, uv_faces = st3d_io.synthesize_uvs(verts), faces.verts_idx.clone()
        noise = torch.randn((size, size, 3), generator=torch.Generator().manual_seed(0))
        tex = (0.5 + 0.1 * noise).clamp(0, 1)
    else:
        uvs, uv_faces = aux.verts_uvs, faces.textures_idx
        tex = next(iter(aux.texture_images.values()))
    tex = tex[None].to(device)
    if resize_texture:
        nchw = F.interpolate(tex.permute(0, 3, 1, 2), size=size, mode='bilinear', align_corners=False)
        tex = nchw.permute(0, 2, 3, 1).contiguous()
    return verts.to(device), faces.verts_idx.to(device), uvs[None].to(device), uv_faces[None].to(device), tex


def vertex_colors_from_map(n_verts, faces, verts_uvs, faces_uvs, texture_map):
    """Initial per-vertex colours from a UV-mapped texture -> (V,3): every vertex takes the map sampled at the UV of its
    first incident corner (the smallest 3 f + j with faces[f, j] == v), with the renderer's sampling conventions (SURVEY.md
    A.3: rows flipped, grid = uv * 2 - 1, bilinear, align_corners=True, border clamp).  A vertex no face uses gets 0.5.
    faces (F,3), verts_uvs (VT,2), faces_uvs (F,3), texture_map (T,T',3).  Done once, in torch."""
    flat = faces.reshape(-1).to(torch.int64)
    n_corners = flat.numel()
    first = torch.full((n_verts,), n_corners, dtype=torch.int64, device=flat.device)
    first.scatter_reduce_(0, flat, torch.arange(n_corners, dtype=torch.int64, device=flat.device), reduce="amin")
    used = first < n_corners
    colors = torch.full((n_verts, 3), 0.5, dtype=torch.float32, device=flat.device)
    if bool(used.any()):
        uv = verts_uvs.reshape(-1, 2).to(torch.float32)[faces_uvs.reshape(-1).to(torch.int64)[first[used]]]
        image = texture_map.reshape(texture_map.shape[-3], texture_map.shape[-2], 3).to(torch.float32)
        nchw = image.flip(0).permute(2, 0, 1)[None]
        grid = (uv * 2.0 - 1.0).reshape(1, 1, -1, 2)
        sampled = F.grid_sample(nchw, grid, mode='bilinear', padding_mode='border', align_corners=True)
        colors[used] = sampled[0, :, 0, :].t()
    return colors


def mean_edge_length(verts, faces):
    """mean length of the unique undirected edges of (verts (V,3), faces (F,3)); once per run, in torch fp64"""
    f = faces.detach().long().cpu()
    he = torch.sort(torch.cat([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]], dim=0), dim=1).values
    e = torch.unique(he, dim=0)
    v = verts.detach().double().cpu()
    return float((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1).mean())


def mesh_regulariser_keys(args, verts, faces, say=print):
    """--laplacian_method / --edge_target_length -> the optional keys of the weights dict that st3d.mesh_losses.mesh_terms
    reads.  A key is present only when its flag is set, so the dict of a default run is what it always was.  'mean' becomes
    the mean edge length of the loaded mesh, computed once and printed."""
    keys = {}
    if getattr(args, "laplacian_method", "uniform") != "uniform":
        keys['mesh_laplacian_method'] = args.laplacian_method
    target = getattr(args, "edge_target_length", 0.0)
    if target == 'mean':
        target = mean_edge_length(verts, faces)
        say(f"Mean edge length of the loaded mesh: {target:.6g} (--edge_target_length mean)")
    if target != 0.0:
        keys['mesh_edge_target_length'] = float(target)
    return keys


def load_scene_vertex(obj_path, device):
    """--texture_type vertex: OBJ -> (verts (V,3), faces (F,3), colours (V,3)) on `device`.  An OBJ with UVs and a texture
    map starts from the map (vertex_colors_from_map); one without -- the case the flag exists for -- from
    (0.5 + 0.1 randn(V,3), seed 0) clamped to [0,1], without a warning: nothing is synthesised that the mesh lacks."""
    verts, faces, aux = st3d_io.load_obj(obj_path)
    if aux.verts_uvs is None or faces.textures_idx is None or not aux.texture_images:
        noise = torch.randn((verts.shape[0], 3), generator=torch.Generator().manual_seed(0))
        colors = (0.5 + 0.1 * noise).clamp(0, 1)
    else:
        colors = vertex_colors_from_map(verts.shape[0], faces.verts_idx, aux.verts_uvs, faces.textures_idx,
                                        next(iter(aux.texture_images.values())))
    return verts.to(device), faces.verts_idx.to(device), colors.to(device)


def atlas_texel_centres(R):
    """The barycentrics (b0, b1) of the centre of every texel of an R x R block -> two (R,R) float64 tensors indexed [y][x]:
    (x + 1/3, y + 1/3) / R where x + y < R, else (R - 1 - x + 2/3, R - 1 - y + 2/3) / R (make_material_atlas's)."""
    y, x = torch.meshgrid(torch.arange(R, dtype=torch.float64), torch.arange(R, dtype=torch.float64), indexing="ij")
    below = x + y < R
    b0 = torch.where(below, x + 1.0 / 3.0, R - 1 - x + 2.0 / 3.0) / R
    b1 = torch.where(below, y + 1.0 / 3.0, R - 1 - y + 2.0 / 3.0) / R
    return b0, b1


def atlas_from_map(R, verts_uvs, faces_uvs, texture_map):
    """Initial atlas from a UV-mapped texture -> (F,R,R,3): the map sampled at the UV of every texel's centre (sum_i b_i uv_i
    over the face's corners, atlas_texel_centres) with the renderer's sampling conventions (rows flipped,
    grid = uv * 2 - 1, bilinear, align_corners=True, border clamp).  verts_uvs (VT,2), faces_uvs (F,3), texture_map
    (T,T',3).  Done once, in torch."""
    b0, b1 = atlas_texel_centres(R)
    b0, b1 = b0.to(torch.float32).to(verts_uvs.device), b1.to(torch.float32).to(verts_uvs.device)
    b2 = 1.0 - b0 - b1
    corner = verts_uvs.reshape(-1, 2).to(torch.float32)[faces_uvs.reshape(-1, 3).to(torch.int64)]        # (F,3,2)
    uv = (b0[None, :, :, None] * corner[:, 0, None, None, :] + b1[None, :, :, None] * corner[:, 1, None, None, :]
          + b2[None, :, :, None] * corner[:, 2, None, None, :])                                         # (F,R,R,2)
    image = texture_map.reshape(texture_map.shape[-3], texture_map.shape[-2], 3).to(torch.float32)
    nchw = image.flip(0).permute(2, 0, 1)[None]
    grid = (uv * 2.0 - 1.0).reshape(1, 1, -1, 2)
    sampled = F.grid_sample(nchw, grid, mode='bilinear', padding_mode='border', align_corners=True)
    return sampled[0, :, 0, :].t().reshape(uv.shape[0], R, R, 3).contiguous()


def load_scene_atlas(obj_path, R, device):
    """--texture_atlas R: OBJ -> (verts (V,3), faces (F,3), atlas (F,R,R,3)) on `device`.  An OBJ with UVs and a texture map
    starts from the map (atlas_from_map); one without -- the case the flag exists for -- from (0.5 + 0.1 randn(F,R,R,3),
    seed 0) clamped to [0,1], without a warning: nothing is synthesised that the mesh lacks."""
    verts, faces, aux = st3d_io.load_obj(obj_path)
    n_faces = faces.verts_idx.shape[0]
    if aux.verts_uvs is None or faces.textures_idx is None or not aux.texture_images:
        noise = torch.randn((n_faces, R, R, 3), generator=torch.Generator().manual_seed(0))
        atlas = (0.5 + 0.1 * noise).clamp(0, 1)
    else:
        atlas = atlas_from_map(R, aux.verts_uvs, faces.textures_idx, next(iter(aux.texture_images.values())))
    return verts.to(device), faces.verts_idx.to(device), atlas.to(device)


def export_atlas_mesh(out_dir, final):
    """What the final export of a --texture_atlas run writes besides the turntable: final.obj (geometry only),
    final_atlas.npy (the clamped texels, st3d.io.load_atlas reads them back) and, while F R^2 <= 2^20, final_colored.obj --
    the atlas as the exact triangle soup it renders as, with ``v x y z r g b`` lines (opens in MeshLab).  -> the line to
    print: what was written, or that the soup was skipped."""
    st3d_io.save_obj(os.path.join(out_dir, "final.obj"), final.verts_packed(), final.faces_packed())
    atlas = final.textures.atlas_packed()
    st3d_io.save_atlas(os.path.join(out_dir, "final_atlas.npy"), atlas)
    n_soup = atlas.shape[0] * atlas.shape[1] * atlas.shape[2]
    if n_soup > st3d_io.ATLAS_SOUP_MAX_FACES:
        return (f"final_colored.obj skipped: the triangle soup of the atlas would have {n_soup} faces (more than "
                f"{st3d_io.ATLAS_SOUP_MAX_FACES}); final_atlas.npy holds the texels")
    sv, sf, sc = st3d_io.atlas_to_triangle_soup(final.verts_packed().cpu(), final.faces_packed().cpu(), atlas.cpu())
    st3d_io.save_obj(os.path.join(out_dir, "final_colored.obj"), sv, sf, verts_colors=sc)
    return f"final_colored.obj: the atlas as a triangle soup of {n_soup} faces"


ViewBatch = namedtuple("ViewBatch", "index size lo hi")      # batch number, its global size, this rank's [lo, hi)


class AsyncImageWriter:
    """PNG dumps off the critical path.  The reference encodes every view of every step on the main thread
    (second_approach.py:183-185: ~30 ms per 512^2 image, 15x the GPU step at config 2).  Here the batch is quantised on
    the GPU exactly like ``tensor_to_image`` (clamp to [0,1], x255, truncate), copied to pinned host memory without
    blocking, and encoded by worker threads once the copy's event has fired; at most `depth` batches are in flight
    (back-pressure instead of unbounded memory).  Pixels are identical; only zlib's effort level is lower."""

    def __init__(self, workers=8, depth=4):
        from concurrent.futures import ThreadPoolExecutor
        self._pool = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="st3d-png")
        self._pending = []
        self._depth = depth

    def submit(self, images, paths):
        """images (n,3,H,W) float on the GPU; paths: n file names."""
        u8 = (images.detach().clamp(0, 1) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        host = torch.empty(u8.shape, dtype=torch.uint8, pin_memory=True)
        host.copy_(u8, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._pending.append([self._pool.submit(self._write, done, host, k, path) for k, path in enumerate(paths)])
        while len(self._pending) > self._depth:
            self._wait(self._pending.pop(0))

    @staticmethod
    def _write(done, host, k, path):
        from PIL import Image
        done.synchronize()
        Image.fromarray(host[k].numpy()).save(path, compress_level=1)

    @staticmethod
    def _wait(futures):
        for f in futures:
            f.result()          # re-raises a failed write

    def flush(self):
        while self._pending:
            self._wait(self._pending.pop(0))


class Run:
    """Everything both drivers need before their loop starts."""

    def __init__(self, args, lr, image_dir):
        import losses as _l
        import style_transfer as _s
        import utils as _u
        self.args = args
        self.rank, self.world, local = st3d_optim.init_distributed()
        if getattr(args, "bake_texture", "off") != "off" and self.world > 1:
            raise RuntimeError(f"--bake_texture cannot run under torch.distributed (world size {self.world}): every rank holds "
                               "only its slice of a batch's views, and sharded baking is not implemented -- run one process")
        if not torch.cuda.is_available():
            raise RuntimeError("st3d needs an MI355X (libst3d has no CPU fallback)")
        self._bake_surface = None           # --bake_texture: texel_surface of the mesh, computed at the first bake (static UVs)
        # one GPU per rank; only a gloo rehearsal (ST3D_DIST_BACKEND=gloo) may put several ranks on one card
        self.device = torch.device(f"cuda:{local % max(torch.cuda.device_count(), 1)}")
        torch.cuda.set_device(self.device)
        _u.device = _s.device = _l.device = self.device
        if args.seed is not None:
            torch.manual_seed(args.seed)
        self.out_dir = args.output_path
        self.image_dir = os.path.join(self.out_dir, image_dir)
        if self.main:
            os.makedirs(self.image_dir, exist_ok=True)
        self.loss_weights = {k: getattr(args, k) for k in (
            'mesh_edge_loss_weight', 'mesh_laplacian_smoothing_weight', 'mesh_normal_consistency_weight',
            'mesh_verts_weight', 'main_loss_weight')}

        self.say("Loading mesh...")
        self.vertex_colors = getattr(args, "texture_type", "uv") == "vertex"
        self.atlas_r = int(getattr(args, "texture_atlas", 0))
        if self.atlas_r:
            verts, faces, tex = load_scene_atlas(args.obj_path, self.atlas_r, self.device)      # tex: the (F,R,R,3) atlas
            self.content_mesh = _u.build_mesh_atlas(tex, verts, faces)
        elif self.vertex_colors:
            verts, faces, tex = load_scene_vertex(args.obj_path, self.device)       # tex: the (V,3) colours
            self.content_mesh = _u.build_mesh_vertex(tex, verts, faces)
        else:
            verts, faces, verts_uvs, faces_uvs, tex = load_scene(args.obj_path, args.size, args.resize_texture, self.device)
            self.content_mesh = _u.build_mesh(verts_uvs, faces_uvs, tex, verts, faces)
        self.original_verts = verts
        self.loss_weights.update(mesh_regulariser_keys(args, verts, faces, self.say))

        cams = FoVPerspectiveCameras(device=self.device)
        supersample = getattr(args, "supersample", 1)
        mip_levels = getattr(args, "texture_mip_levels", 1)
        if mip_levels != 1:
            settings = RasterizationSettings(image_size=args.size, blur_radius=0.0, faces_per_pixel=1,
                                             texture_mip_levels=mip_levels,
                                             texture_lod_bias=getattr(args, "texture_lod_bias", 0.0))
        elif supersample == 1:
            settings = RasterizationSettings(image_size=args.size, blur_radius=0.0, faces_per_pixel=1)
        else:
            settings = RasterizationSettings(image_size=args.size, blur_radius=0.0, faces_per_pixel=1, supersample=supersample)
        lights, materials = make_lights(args, self.device)
        self.renderer = MeshRenderer(rasterizer=MeshRasterizer(cameras=cams, raster_settings=settings),
                                     shader=SoftPhongShader(device=self.device, cameras=cams, lights=lights,
                                                            materials=materials))
        self.say("Loading model...")
        self.vgg = _u.get_vgg(weights=args.vgg_weights)

        self.say("Building cameras...")
        gen = torch.Generator().manual_seed(args.seed) if args.seed is not None else None
        if getattr(args, "view_selection", "random") == "coverage":
            self.cameras = self.select_views(gen)
        else:
            self.cameras = (_u.build_random_cameras(args.n_views, generator=gen) if args.randomize_views
                            else _u.build_fixed_cameras(args.n_views))
        if self.world > 1:                      # every rank must look through the same cameras
            torch.distributed.broadcast(self.cameras.R, 0)
            torch.distributed.broadcast(self.cameras.T, 0)

        # one optimiser (one Adam state) for the whole run, over all view batches
        levels = getattr(args, "texture_pyramid_levels", 1)
        diffusion = float(getattr(args, "verts_diffusion", 0.0))
        if diffusion:
            self.opt = _u.setup_optimizations(args.optimization_target, self.content_mesh, lr, texture_pyramid_levels=levels,
                                              verts_diffusion=diffusion)
        elif levels == 1:
            self.opt = _u.setup_optimizations(args.optimization_target, self.content_mesh, lr)
        else:
            self.opt = _u.setup_optimizations(args.optimization_target, self.content_mesh, lr, texture_pyramid_levels=levels)
        self.pyramid = self.opt.get('texture_pyramid')      # None: the texture is the plain leaf opt['texture_map']
        self.diffusion = self.opt.get('verts_diffusion')    # None: the vertices are the plain leaf opt['verts']
        self._diffusion_warned = False
        if self.diffusion is not None:
            self.say(f"Vertex diffusion: lambda {self.diffusion.lam:g}, largest degree {self.diffusion.max_degree}, at most "
                     f"{self.diffusion.max_iter} CG iterations per solve at tol {self.diffusion.tol:g}")
            if args.verts_lr is not None:       # --verts_lr is the step size of u, whether or not a texture is optimised too
                groups = [{"params": [self.diffusion.params], "lr": args.verts_lr, "uniform": True}]
                if args.optimization_target == 'both':
                    texture_leaf = self.pyramid.params if self.pyramid is not None else self.opt[self.texture_key]
                    groups.append({"params": [texture_leaf], "lr": lr})
                self.opt['optimizer'] = st3d_optim.Adam(groups)
        elif args.verts_lr is not None and args.optimization_target == 'both':
            texture_leaf = self.pyramid.params if self.pyramid is not None else self.opt[self.texture_key]
            self.opt['optimizer'] = st3d_optim.Adam([{"params": [self.opt['verts']], "lr": args.verts_lr},
                                                     {"params": [texture_leaf], "lr": lr}])
        self.optimizer = self.opt['optimizer']
        self.original_map = tex
        self.chamfer_generator = self.chamfer_target = None
        if getattr(args, "chamfer_weight", 0.0):        # off (the default): nothing runs, no generator is created
            self.setup_chamfer()
        self.swd_generator = None
        if getattr(args, "swd_weight", 0.0):            # off (the default): nothing runs, no generator is created
            self.swd_generator = torch.Generator().manual_seed(args.seed if args.seed is not None else 0)
        self.style_scales = tuple(getattr(args, "style_scales", None) or (1,))
        self.style_scale_weights = getattr(args, "style_scale_weights", None)
        if self.multi_scale:            # the default: nothing is said, nothing runs
            weights = self.style_scale_weights or (1.0,) * len(self.style_scales)
            self.say("Style scales: " + ", ".join(f"1/{f} (plan side {args.size // f}, weight {w:g})"
                                                   for f, w in zip(self.style_scales, weights)))
        self.lap_pools = None
        if getattr(args, "lap_weight", 0.0):        # off (the default): nothing is said, nothing runs
            from . import lap as st3d_lap
            self.lap_pools = st3d_lap.check_pools(getattr(args, "lap_pools", None) or LAP_POOLS_DEFAULT, args.size)
            st3d_lap.reserve_cache(len(self.lap_pools) * -(-args.n_views // args.batch_size))
            self.say("Laplacian content term: weight %g, " % args.lap_weight
                     + ", ".join(f"pool {p} (pooled side {args.size // p})" for p in self.lap_pools))
        self.color_mode = getattr(args, "preserve_color", "off")
        self._utils = _u
        matched_style = None
        if self.color_mode != "off":        # the default: nothing is said, nothing runs.  Before --resume is read: a resumed
            matched_style = self.setup_color()      # run sees the same style image
        self.regions = None
        if getattr(args, "style_regions", None) is not None:    # the default: nothing is said, nothing runs.  Before --resume
            self.setup_regions(verts, faces)                    # is read: a resumed run must name the same regions
        self.progress = 0               # epochs (second approach) / view batches (first approach) already done
        if args.resume:
            self.load_checkpoint(args.resume)
        self.style_image = _u.load_as_tensor(args.style_path, size=args.size)   # loop-invariant; the reference reloads it
        if matched_style is not None:
            self.style_image = matched_style
        self._log = os.path.join(self.out_dir, 'log.txt')
        if self.main:
            with open(self._log, 'w') as fh:
                fh.write('Logger:\n')
        self.writer = AsyncImageWriter()

    # ---- small helpers
    @property
    def texture_key(self):
        """the entry of self.opt that holds the colour leaf: the map, the (V,3) colours of a --texture_type vertex run or the
        (F,R,R,3) texels of a --texture_atlas run"""
        if self.atlas_r:
            return 'atlas'
        return 'verts_features' if self.vertex_colors else 'texture_map'

    @property
    def main(self):
        return self.rank == 0

    @property
    def multi_scale(self):
        """--style_scales / --style_scale_weights ask for anything but the single-scale loss"""
        return self.style_scales != (1,) or self.style_scale_weights is not None

    @property
    def style_color(self):
        """style_transfer's ``color``: 'luminance' under --preserve_color luminance, else 'rgb' (today's loop)"""
        return 'luminance' if getattr(self, "color_mode", "off") == "luminance" else 'rgb'

    def say(self, msg):
        if self.main:
            print(msg)

    def log(self, line):
        self.check_diffusion()          # the caller has just read the loss back: the solves behind it are finished
        if self.main:
            with open(self._log, 'a') as fh:
                fh.write(line + '\n')

    def setup_color(self):
        """--preserve_color match / luminance: the moments of the LOADED mesh as the run sees it -- every rank renders it
        through all n_views cameras in batches of batch_size under no_grad and takes st3d.color's 10 sums over the covered
        pixels, added over the batches in fp64 in batch order -- and the style image prepared from them: 'match' recolours
        it to the content's mean and covariance (match_matrix), 'luminance' takes its luminance and matches that to the
        content's luminance (luma_match).  Every rank computes the same bits: no communication.  Rank 0 writes
        style_matched.png; one line of figures.  -> the (3,size,size) style image of the run."""
        import numpy as np
        from . import color as _color
        a, u = self.args, self._utils
        luminance = self.color_mode == "luminance"
        if luminance:       # loss_images() asks luma_cached for every view batch's content in turn: all of them must fit
            _color.reserve_cache(math.ceil(a.n_views / a.batch_size) + 1)
        style = u.load_as_tensor(a.style_path, size=a.size)[None]
        sums = np.zeros(10, np.float64)
        with torch.no_grad():
            for first in range(0, a.n_views, a.batch_size):
                cams = self.cameras[first:min(first + a.batch_size, a.n_views)]
                img, cov = u.render_meshes(self.renderer, self.content_mesh, cams)
                if luminance:
                    img = _color.luma_fwd(img)
                sums += _color.color_sums(img, (cov > 0).reshape(img.shape[0], -1)).cpu().numpy()
            content = _color.stats_from_sums(sums)
            if luminance:
                style = _color.luma_fwd(style)
                before = _color.color_stats(style)
                k, b = _color.luma_match(before, content)
                matched = _color.recolor(style, np.eye(3) * k, np.full(3, b))
            else:
                before = _color.color_stats(style)
                matched = _color.recolor(style, *_color.match_matrix(before, content))
            after = _color.color_stats(matched)
        fmt = lambda m: "(" + ", ".join(f"{v:.4f}" for v in m) + ")"
        self.say(f"Preserve colour ({self.color_mode}): content mean {fmt(content['mean'])} over {content['n']} covered pixels "
                 f"of {a.n_views} views; style mean {fmt(before['mean'])} -> {fmt(after['mean'])}")
        if self.main:
            u.tensor_to_image(matched).save(os.path.join(self.out_dir, 'style_matched.png'))
        return matched[0].contiguous()

    def setup_regions(self, verts, faces):
        """--style_regions: the labels of the LOADED mesh (validated once, here), one style image per region, and -- from the
        fragments of the loaded mesh through all n_views cameras, rasterised once in batches of batch_size -- each region's
        share of the covered pixels and the debug pictures regions/view_k.png (rank 0).  Refused under torch.distributed
        with several ranks: the sharded sums of the term are not implemented."""
        from . import ops as _ops
        from . import regions as _regions
        from . import render as _render
        a, u = self.args, self._utils
        if self.world > 1:
            raise RuntimeError(f"--style_regions cannot run under torch.distributed (world size {self.world}): the per-region "
                               "sums of a sharded batch are not implemented -- run one process")
        parsed = _regions.parse_spec(a.style_regions)
        materials = st3d_io.load_obj(a.obj_path, load_textures=False)[1].materials_idx if parsed[0] == "material" else None
        labels = _regions.labels_from_spec(parsed, verts, faces, materials)
        face_regions, R = _regions.check_face_regions(labels, int(faces.shape[0]), device=self.device)
        if len(a.region_styles) != R:
            raise ValueError(f"--style_regions {a.style_regions} makes {R} regions on {a.obj_path} but --region_styles names "
                             f"{len(a.region_styles)} images: exactly one per region")
        weights = getattr(a, "region_style_weights", None)
        if weights is not None and len(weights) != R:
            raise ValueError(f"--region_style_weights must give one weight per region ({R}), got {len(weights)}")
        styles = torch.stack([u.load_as_tensor(p, size=a.size) for p in a.region_styles]).contiguous()
        self.regions = {"spec": a.style_regions, "R": R, "labels": face_regions, "styles": styles,
                        "weights": tuple(float(w) for w in weights) if weights is not None else None, "planes": {}}
        faces_i32, sums = self.content_mesh.faces_i32(), []
        v32 = verts.detach().to(torch.float32).contiguous()
        if self.main:
            os.makedirs(os.path.join(self.out_dir, "regions"), exist_ok=True)
        with torch.no_grad():
            for first in range(0, a.n_views, a.batch_size):
                Rm, T = _render.join_cameras(self.cameras[first:min(first + a.batch_size, a.n_views)])
                p2f = _ops.raster_fwd(_ops.project_verts(v32, Rm.to(self.device), T.to(self.device)), faces_i32, a.size)[0]
                sums.append(_regions.region_planes(p2f, face_regions, R)[1])
                if self.main:
                    for k, img in enumerate(_regions.region_preview(p2f, face_regions)):
                        u.tensor_to_image(img).save(os.path.join(self.out_dir, "regions", f"view_{first + k}.png"))
        shares = _regions.region_shares(sums)
        self.say(f"Style regions ({a.style_regions}): R = {R}; share of the covered pixels over {a.n_views} views: "
                 + ", ".join(f"region {r} {100.0 * s:.1f} %" + (f" (weight {self.regions['weights'][r]:g})"
                                                                 if weights is not None else "")
                             for r, s in enumerate(shares)))

    def region_loss(self, current, content, mesh, vb):
        """--style_regions: compute_second_approach_loss with the per-region style term in the perceptual term's place.  The
        planes come from the fragments of the step's own render (regions.fragments_of: the render's backward keeps them, the
        rasteriser's FragmentCache entry when the view came from it) -- nothing is rasterised a second time; with
        --optimization_target texture the planes of a view batch are built once and kept, with moving vertices every step."""
        import losses as _l
        from . import regions as _regions
        a, g = self.args, self.regions
        fixed = a.optimization_target == 'texture'
        planes = g["planes"].get((vb.index, vb.lo, vb.hi)) if fixed else None
        if planes is None:
            p2f = _regions.fragments_of(current)
            if p2f is None or tuple(p2f.shape) != (current.shape[0], current.shape[2], current.shape[3]):
                raise RuntimeError("--style_regions: the render of this step kept no one-face-per-pixel fragments to label")
            planes = _regions.region_planes(p2f, g["labels"], g["R"])
            if fixed:
                g["planes"][(vb.index, vb.lo, vb.hi)] = planes
        perceptual = _l.compute_region_style_loss(current, content, g["styles"], None, g["labels"], self.vgg,
                                                  style_weight=a.style_weight, content_weight=a.content_weight,
                                                  region_weights=g["weights"], batch_denom=vb.size, planes=planes)
        if a.optimization_target == 'texture':
            return perceptual                               # no main_loss_weight here, as compute_second_approach_loss
        return self.loss_weights['main_loss_weight'] * perceptual + _l._mesh_terms(self.opt['verts'], self.original_verts, mesh,
                                                                                   self.loss_weights)

    def loss_images(self, current, content):
        """-> the (current, content) pair to hand the style terms: the inputs themselves, or under --preserve_color luminance
        their luminance -- luma(current), which carries the render's need / flat / epoch tags to the loss, and
        luma_cached(content), the same tensor every step.  The TV term and the view dumps keep the RGB `current`."""
        if self.color_mode != "luminance":
            return current, content
        from . import color as _color
        return _color.luma(current), _color.luma_cached(content)

    def recombine_leaf(self, mesh):
        """--preserve_color luminance at export: `mesh` with its colour carrier (the map, the pyramid's synthesised map, the
        vertex colours or the atlas) replaced by its luminance under the chroma of the loaded one (color.recombine_texture).
        A texel that never moved has d = 0 and keeps its loaded value.  One line says how many texels changed."""
        from . import color as _color
        u, tex = self._utils, mesh.textures
        with torch.no_grad():
            if self.atlas_r:
                leaf = tex.atlas_packed()
            elif self.vertex_colors:
                leaf = tex.verts_features_packed()
            else:
                leaf = tex.maps_padded()
            original = self.original_map.reshape(leaf.shape)
            out = _color.recombine_texture(leaf, original)
            changed = int((out != original).any(dim=-1).sum())
        self.say(f"Recombine: {changed} of {out.numel() // 3} texels carry a new luminance under their loaded chroma "
                 "(--preserve_color luminance)")
        if self.atlas_r:
            return u.build_mesh_atlas(out, mesh.verts_packed(), mesh.faces_packed())
        if self.vertex_colors:
            return u.build_mesh_vertex(out, mesh.verts_packed(), mesh.faces_packed())
        return u.build_mesh(tex.verts_uvs_padded(), tex.faces_uvs_padded(), out, mesh.verts_packed(), mesh.faces_packed())

    def select_views(self, generator):
        """--view_selection coverage: n_views of --view_candidates random directions, picked greedily by the texels they add
        (utils.build_coverage_cameras) on the loaded mesh at --size; one line of figures and texel_coverage.png."""
        import utils as _u
        args = self.args
        cameras, report = _u.build_coverage_cameras(args.n_views, self.content_mesh, args.size,
                                                    candidates=args.view_candidates, generator=generator)
        self.say(f"View selection: the {args.n_views} picked of {report['candidates']} candidates reach {report['picked']} of "
                 f"the {report['pool']} texels the candidates reach together; the first {args.n_views} candidates reach "
                 f"{report['first_n']}")
        if self.main:
            share = report['counts'].to(torch.float32) / float(args.n_views)
            _u.tensor_to_image(share[None].expand(3, -1, -1)).save(os.path.join(self.out_dir, 'texel_coverage.png'))
        return cameras

    def bake_targets(self, targets, cams, label):
        """--bake_texture: bake the batch's stylised views `targets` (n,3,size,size), seen through `cams` on the current
        vertices, into the texture leaf: baked_texture(acc, fallback = the leaf), in place under no_grad.  Stateless per
        batch: Adam's moments and the checkpoints know nothing of it.  One line says how many texels were written.  With the
        flag off (the default) nothing runs."""
        a = self.args
        mode = getattr(a, "bake_texture", "off")
        if mode == "off" or targets is None or cams is None or len(cams) == 0:
            return
        from . import bake as _bake
        leaf = self.opt['texture_map']
        with torch.no_grad():
            mesh = self.current_mesh()
            if self._bake_surface is None:
                tex = mesh.textures
                uvs = tex.verts_uvs_padded().detach().to(torch.float32).reshape(-1, 2).contiguous()
                self._bake_surface = _bake.texel_surface(uvs, tex.faces_uvs_i32(), int(leaf.shape[-2]))
            texture, acc = self._utils.bake_texture(mesh, targets, cams, a.size, mode=mode, power=a.bake_power,
                                                    min_cos=a.bake_min_cos, surface=self._bake_surface)
            leaf.copy_(texture.reshape(leaf.shape))
            written = int((acc[..., 3] > 0).sum())
        self.say(f"Bake ({label}): {written} of {acc.shape[0] * acc.shape[1]} texels written from {len(cams)} views "
                 f"(--bake_texture {mode})")

    def check_diffusion(self):
        """--verts_diffusion: warn, once per run, when the latest forward or backward solve stopped at its iteration cap."""
        dv = getattr(self, "diffusion", None)
        if dv is None or self._diffusion_warned:
            return
        for name, info in (("forward", dv.last_info()), ("backward", dv.last_info(backward=True))):
            if info is not None and not all(info["converged"]):
                self._diffusion_warned = True
                self.say(f"WARNING: the {name} solve of --verts_diffusion stopped after {max(info['iterations'])} iterations "
                         f"at a relative residual of {max(info['residual']):.3g} (tol {dv.tol:g}); not reported again")
                return

    def save_views(self, images, first_index):
        """view_<k>.png for this rank's views of the batch, k counted over the whole view set (asynchronous)."""
        self.writer.submit(images, [os.path.join(self.image_dir, f"view_{first_index + j}.png") for j in range(images.shape[0])])

    def current_mesh(self):
        o = self.opt
        if getattr(self, "diffusion", None) is not None:    # one forward solve per step: the mesh, the regularisers and the
            o['verts'] = self.diffusion.verts()             # silhouette / Chamfer terms all read this tensor
        if self.atlas_r:
            return self._utils.build_mesh_atlas(o['atlas'], o['verts'], o['faces'])
        if self.vertex_colors:
            return self._utils.build_mesh_vertex(o['verts_features'], o['verts'], o['faces'])
        texture = self.pyramid.texture() if self.pyramid is not None else o['texture_map']      # synthesised every step
        return self._utils.build_mesh(o['verts_uvs'], o['faces_uvs'], texture, o['verts'], o['faces'])

    def batches(self):
        """The reference's schedule (ceil(n_views / batch_size) consecutive slices) with this rank's share of each."""
        n, bs = self.args.n_views, self.args.batch_size
        for i in range(math.ceil(n / bs)):
            first, size = i * bs, min((i + 1) * bs, n) - i * bs
            lo, hi = st3d_optim.shard_views(size, self.rank, self.world)
            yield ViewBatch(i, size, first + lo, first + hi)

    def zero_contribution(self):
        """A rank without views in this batch still joins the gradient all-reduce (with zeros)."""
        for p in self.optimizer.params:
            p.grad = torch.zeros_like(p)

    def idle_contribution(self):
        """This rank has no views in the batch: it still joins the gradient all-reduce, and it still owes its 1/world
        share of the view-INDEPENDENT terms (the mesh regularisers of 'mesh'/'both' and the optional texture
        regularisers), which every rank adds with weight 1/world so that the SUM over ranks counts them once.
        Leaves the gradients in place for ``optimizer.step()`` and returns this rank's (detached) loss share."""
        import losses as _l
        self.zero_contribution()
        mesh = self.current_mesh()
        total = self.regularisers(None, None, mesh, 0, 1)
        if self.args.optimization_target in ('mesh', 'both'):
            total = total + _l._mesh_terms(self.opt['verts'], self.original_verts, mesh, self.loss_weights)
        total = total + self.chamfer_term(mesh)      # view-independent too; the draw keeps this rank's generator in step
        if torch.is_tensor(total) and total.requires_grad:
            total.backward()                      # accumulates into the zero gradients
        return total.detach() if torch.is_tensor(total) else torch.zeros((), device=self.device)

    def global_sum(self, value):
        t = value.detach().clone()
        if self.world > 1:
            torch.distributed.all_reduce(t)
        return t

    # ---- checkpoint / resume: parameters + Adam moments + how far the run got
    def save_checkpoint(self, progress):
        if not self.main:
            return
        if self.pyramid is None:
            texture = self.opt[self.texture_key]
        else:
            with torch.no_grad():
                texture = self.pyramid.texture()
        blob = {"progress": int(progress), "optimization_target": self.args.optimization_target,
                "texture_type": "vertex" if self.vertex_colors else "uv", "texture_atlas": self.atlas_r,
                self.texture_key: texture.detach().cpu(), "verts": self.opt['verts'].detach().cpu(),
                "optimizer": self.optimizer.state_dict()}
        if getattr(self, "diffusion", None) is not None:    # u is the state of record; "verts" is what it stood for when last solved
            blob["verts_diffusion"] = self.diffusion.params.detach().cpu()
            blob["verts_diffusion_lambda"] = float(self.diffusion.lam)
        if self.pyramid is not None:        # the flat parameters are the state of record; texture_map is what they sum to
            blob["texture_pyramid"] = self.pyramid.params.detach().cpu()
            blob["texture_pyramid_levels"] = self.pyramid.levels
        generator = getattr(self, "chamfer_generator", None)
        if generator is not None:           # --chamfer_weight: where the point draws of the run have got to
            blob["chamfer_generator_state"] = generator.get_state().cpu()
        generator = getattr(self, "swd_generator", None)
        if generator is not None:           # --swd_weight: where the direction draws of the run have got to
            blob["swd_generator_state"] = generator.get_state().cpu()
        if getattr(self, "multi_scale", False):     # --style_scales: no state of its own, but Adam's moments belong to that loss
            blob["style_scales"] = list(self.style_scales)
            blob["style_scale_weights"] = list(self.style_scale_weights) if self.style_scale_weights is not None else None
        if getattr(self, "lap_pools", None) is not None:    # --lap_weight: no state of its own, but Adam's moments belong to that loss
            blob["lap_pools"] = list(self.lap_pools)
        if getattr(self, "color_mode", "off") != "off":     # --preserve_color: Adam's moments belong to that style image and loss
            blob["preserve_color"] = self.color_mode
        if getattr(self, "regions", None) is not None:      # --style_regions: Adam's moments belong to these regions' loss
            blob["style_regions"] = {"spec": self.regions["spec"], "R": self.regions["R"],
                                     "weights": list(self.regions["weights"]) if self.regions["weights"] is not None else None}
        tmp =os.path.join(self.out_dir, "checkpoint.pt.tmp")
        torch.save(blob, tmp)
        os.replace(tmp, os.path.join(self.out_dir, "checkpoint.pt"))

    def load_checkpoint(self, path):
        blob = torch.load(path, map_location="cpu", weights_only=True)
        if blob["optimization_target"] != self.args.optimization_target:
            raise ValueError("checkpoint was written for optimization_target=%r" % blob["optimization_target"])
        have_type, want_type = blob.get("texture_type", "uv"), "vertex" if self.vertex_colors else "uv"
        if have_type != want_type:
            raise ValueError("checkpoint was written with --texture_type %s, this run has %s" % (have_type, want_type))
        have_atlas = int(blob.get("texture_atlas", 0))
        if have_atlas != self.atlas_r:
            raise ValueError("checkpoint was written with --texture_atlas %d, this run has %d" % (have_atlas, self.atlas_r))
        have = int(blob.get("texture_pyramid_levels", 1))
        want = self.pyramid.levels if self.pyramid is not None else 1
        if have != want:
            raise ValueError("checkpoint was written with %d texture pyramid level(s), this run has %d" % (have, want))
        dv = getattr(self, "diffusion", None)
        have_lam, want_lam = float(blob.get("verts_diffusion_lambda", 0.0)), dv.lam if dv is not None else 0.0
        if have_lam != want_lam:
            raise ValueError("checkpoint was written with --verts_diffusion %g, this run has %g" % (have_lam, want_lam))
        generator = getattr(self, "chamfer_generator", None)
        if ("chamfer_generator_state" in blob) != (generator is not None):
            raise ValueError("checkpoint was written %s --chamfer_weight, this run is %s it"
                             % (("with", "without") if "chamfer_generator_state" in blob else ("without", "with")))
        if generator is not None:
            generator.set_state(blob["chamfer_generator_state"])
        generator = getattr(self, "swd_generator", None)
        if ("swd_generator_state" in blob) != (generator is not None):
            raise ValueError("checkpoint was written %s --swd_weight, this run is %s it"
                             % (("with", "without") if "swd_generator_state" in blob else ("without", "with")))
        if generator is not None:
            generator.set_state(blob["swd_generator_state"])
        want_weights = getattr(self, "style_scale_weights", None)
        have_scales = (tuple(blob.get("style_scales", (1,))), blob.get("style_scale_weights"))
        want_scales = (tuple(getattr(self, "style_scales", (1,))), list(want_weights) if want_weights is not None else None)
        if have_scales != want_scales:
            raise ValueError("checkpoint was written with --style_scales %s (weights %s), this run has %s (weights %s)"
                             % (have_scales + want_scales))
        have_pools, want_pools = blob.get("lap_pools"), getattr(self, "lap_pools", None)
        if (list(have_pools) if have_pools is not None else None) != (list(want_pools) if want_pools is not None else None):
            described = lambda q: "no --lap_weight" if q is None else "--lap_weight and --lap_pools %s" % ",".join(str(p) for p in q)
            raise ValueError("checkpoint was written with %s, this run has %s" % (described(have_pools), described(want_pools)))
        have_color, want_color = blob.get("preserve_color", "off"), getattr(self, "color_mode", "off")
        if have_color != want_color:
            raise ValueError("checkpoint was written with --preserve_color %s, this run has %s" % (have_color, want_color))
        g = getattr(self, "regions", None)
        have_regions = blob.get("style_regions")
        want_regions = None if g is None else {"spec": g["spec"], "R": g["R"],
                                               "weights": list(g["weights"]) if g["weights"] is not None else None}
        if have_regions != want_regions:
            described = lambda d: "no --style_regions" if d is None else "--style_regions %s (R = %d, weights %s)" % (
                d["spec"], d["R"], d["weights"])
            raise ValueError("checkpoint was written with %s, this run has %s" % (described(have_regions), described(want_regions)))
        with torch.no_grad():
            if self.pyramid is not None:
                self.pyramid.load_params(blob["texture_pyramid"].to(self.device))
            else:
                self.opt[self.texture_key].copy_(blob[self.texture_key])
            if dv is not None:
                dv.load_params(blob["verts_diffusion"].to(self.device))     # opt['verts'] is solved for again by current_mesh()
            else:
                self.opt['verts'].copy_(blob["verts"])
        self.optimizer.load_state_dict(blob["optimizer"])
        self.progress = int(blob["progress"])
        self.say(f"Resumed from {path} at {self.progress}")

    def maybe_checkpoint(self, done):
        every = self.args.checkpoint_every
        if every and done % every == 0:
            self.save_checkpoint(done)

    def regularisers(self, current, coverage, mesh, n_local, batch_size):
        """Optional extra terms (all weights default to 0 = reference behaviour).  The image term is a per-view mean and
        is weighted by this rank's share of the batch; the texture terms are view-independent and enter once over all
        ranks (the gradient all-reduce SUMs)."""
        import losses as _l
        a, total = self.args, 0
        if getattr(a, "tv_weight", 0.0) and n_local:
            total = total + a.tv_weight * (n_local / batch_size) * _l.compute_tv_loss(current, coverage)
        if getattr(a, "rgb_range_weight", 0.0):
            total = total + (a.rgb_range_weight / self.world) * _l.rgb_range_loss(mesh)
        if getattr(a, "texture_l2_weight", 0.0):
            total = total + (a.texture_l2_weight / self.world) * _l.texture_l2_loss(mesh, self.original_map)
        return total

    def silhouette_term(self, mesh, cams, target, batch_size):
        """--silhouette_weight x this rank's share of the batch mean of (soft silhouette of `mesh` - target)^2; target = the
        0/1 coverage of the content renders of the same views.  An image term like tv_weight: divided by the GLOBAL batch,
        nothing on a rank without views, and with weight 0 (the default) nothing runs at all."""
        import losses as _l
        a = self.args
        if not getattr(a, "silhouette_weight", 0.0) or cams is None or len(cams) == 0:
            return 0
        return a.silhouette_weight * _l.compute_silhouette_loss(self.renderer, mesh, cams, target,
                                                                sigma=a.silhouette_sigma, batch_denom=batch_size,
                                                                faces_per_pixel=getattr(a, "silhouette_faces_per_pixel", None))

    def nnfm_term(self, current, cov, style, batch_size):
        """--nnfm_weight x this rank's share of the batch mean of the NNFM style term of the `current` renders against
        `style` over --nnfm_layers (losses.compute_nnfm_loss).  An image term like tv_weight: divided by the GLOBAL batch, so
        a sharded run equals the unsharded one; nothing on a rank without views; --style_mask object hands the renders'
        coverage `cov` to it as position weights.  With weight 0 (the default) nothing runs at all.  No checkpoint state."""
        a = self.args
        if not getattr(a, "nnfm_weight", 0.0) or current is None or current.shape[0] == 0:
            return 0
        import losses as _l
        masks = cov if getattr(a, "style_mask", "none") == 'object' else None
        return a.nnfm_weight * _l.compute_nnfm_loss(current, style, self.vgg, layers=a.nnfm_layers, masks=masks,
                                                    batch_denom=batch_size)

    def lap_term(self, seen, seen_content, batch_size):
        """--lap_weight x this rank's share of the batch mean of the Laplacian content term of the renders `seen` against the
        content renders `seen_content` over --lap_pools (losses.compute_laplacian_loss) -- both as the other terms see them
        (loss_images: the luminance under --preserve_color luminance).  An image term like nnfm_term: divided by the GLOBAL
        batch, nothing on a rank without views, and with weight 0 (the default) nothing runs at all.  The term stays at full
        resolution.  Checkpoints record the pools (lap_pools)."""
        a = self.args
        if not getattr(a, "lap_weight", 0.0) or seen is None or seen.shape[0] == 0:
            return 0
        import losses as _l
        return a.lap_weight * _l.compute_laplacian_loss(seen, seen_content, self.lap_pools, batch_denom=batch_size)

    def swd_term(self, current, cov, style, batch_size):
        """--swd_weight x this rank's share of the batch mean of the sliced Wasserstein style term of the `current` renders
        against `style` over --swd_layers (losses.compute_swd_loss), scaled like nnfm_term: divided by the GLOBAL batch, and
        --style_mask object hands it the renders' coverage.  The step's directions come from the run's generator (seeded with
        --seed, 0 when unset, identically on every rank; kept in checkpoints as swd_generator_state).  A rank without views
        adds nothing but still makes the draw, so that every rank projects onto the same directions in every step.  With
        weight 0 (the default) nothing runs at all."""
        a = self.args
        generator = getattr(self, "swd_generator", None)
        if not getattr(a, "swd_weight", 0.0) or generator is None:
            return 0
        import style_transfer as _st
        directions = _st.swd_draw(a.swd_layers, a.swd_directions, generator)
        if current is None or current.shape[0] == 0:
            return 0
        import losses as _l
        masks = cov if getattr(a, "style_mask", "none") == 'object' else None
        return a.swd_weight * _l.compute_swd_loss(current, style, self.vgg, layers=a.swd_layers, directions=directions,
                                                  masks=masks, batch_denom=batch_size)

    def setup_chamfer(self):
        """--chamfer_weight > 0: the run's generator, seeded with --seed (0 when unset) identically on every rank, and the
        target cloud -- --chamfer_samples points sampled once from the loaded mesh, before any checkpoint is read, so that a
        resumed run holds the same target.  Prints N, the surface area and the level the term settles at."""
        from . import mesh_losses as _ml
        a = self.args
        self.chamfer_generator = torch.Generator(device=self.device)
        self.chamfer_generator.manual_seed(a.seed if a.seed is not None else 0)
        with torch.no_grad():
            self.chamfer_target = _ml.sample_points_from_meshes(self.content_mesh, a.chamfer_samples,
                                                                generator=self.chamfer_generator).detach()
        area = _ml.surface_area(self.content_mesh)
        self.say(f"Chamfer term: {a.chamfer_samples} points per cloud, surface area {area:.6g}, expected floor 2A/(pi N) = "
                 f"{_ml.chamfer_floor(area, a.chamfer_samples):.6g} (the term is not 0 at its optimum)")

    def chamfer_term(self, mesh):
        """--chamfer_weight / world x chamfer_distance(--chamfer_samples points redrawn from `mesh`, the target cloud).  The
        term is view-independent like mesh_terms: every rank draws the same points from the same generator state and adds
        1/world of the same value, so the summed gradient counts it once.  With weight 0 (the default) nothing runs."""
        if getattr(self, "chamfer_generator", None) is None:
            return 0
        from . import mesh_losses as _ml
        a = self.args
        points = _ml.sample_points_from_meshes(mesh, a.chamfer_samples, generator=self.chamfer_generator)
        return (a.chamfer_weight / self.world) * _ml.chamfer_distance(points, self.chamfer_target)[0]

    def fill_unseen(self, mesh, final):
        """--fill_unseen chart / map: the texels of `mesh`'s unclamped map whose bits are still the loaded map's never moved;
        they are filled in the clamped map of `final` from the texels that did (utils.fill_texture) -> the mesh to export.
        One line of figures and texel_filled.png (white = filled).  Rank 0 only, like the export itself."""
        u, mode = self._utils, self.args.fill_unseen
        filled, report = u.fill_texture(final, self.original_map, mode, moved_from=mesh)
        where = "chart and gutter" if mode == "chart" else "map"
        self.say(f"Fill: {report['filled']} of the {report['domain']} texels of the {where} never moved and were filled "
                 f"({report['moved']} texels moved; --fill_unseen {mode})")
        u.tensor_to_image(report['mask'].to(torch.float32)[None].expand(3, -1, -1)).save(
            os.path.join(self.out_dir, 'texel_filled.png'))
        return filled

    def export(self, mesh):
        """final_render/view_k.png from 12 turntable cameras + final.obj/.mtl/.png (first_approach.py:219-225)."""
        from . import ops as _ops
        self.writer.flush()
        _ops.check_near_plane(block=True)       # a mesh that reached the near clipping plane fails loudly (no clipping at K = 1)
        if self.main:
            u = self._utils
            # --preserve_color luminance: recombine -> clamp -> --fill_unseen (which still reads what moved off the
            # un-recombined mesh: a texel that never moved keeps its loaded bits either way)
            final = u.finalize_mesh(self.recombine_leaf(mesh) if getattr(self, "color_mode", "off") == "luminance" else mesh)
            if getattr(self.args, "fill_unseen", "off") != "off":
                final = self.fill_unseen(mesh, final)
            u.save_render(self.renderer, final, u.build_fixed_cameras(12), os.path.join(self.out_dir, "final_render"))
            tex = final.textures
            if self.atlas_r:
                self.say(export_atlas_mesh(self.out_dir, final))
            elif self.vertex_colors:        # v x y z r g b lines; no MTL, no PNG
                st3d_io.save_obj(os.path.join(self.out_dir, "final.obj"), final.verts_packed(), final.faces_packed(),
                                 verts_colors=tex.verts_features_packed())
            else:
                st3d_io.save_obj(os.path.join(self.out_dir, "final.obj"), final.verts_packed(), final.faces_packed(),
                                 tex.verts_uvs_padded()[0], tex.faces_uvs_padded()[0], tex.maps_padded()[0])
        if self.world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
