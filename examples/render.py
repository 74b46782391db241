#!/usr/bin/env python3
"""Mesh -> views on the MI355X path: shaded, depth, normal and (optionally) contour PNGs of an OBJ file from orbit cameras.

    python -m examples.render mesh.obj --views 8 --size 512 --out DIR [--contours] [--smooth] [--mode orthographic]
    python -m examples.render mesh.obj --out DIR --clip_text "a long dress" --clip_weights clip_vit_b32.pt --bpe_path bpe_simple_vocab_16e6.txt.gz
    python -m examples.render mesh.obj --out DIR --clip_image photo.png --clip_weights clip_vit_b32.pt

No reference counterpart (the reference looks at its meshes in open3d / pymeshlab windows).  The meshes of examples/generate.py
and examples/reconstruct.py live in [-1, 1]^3, which the default cameras (distance 2.6, 40 degrees) frame.  ``--clip_text`` /
``--clip_image`` print the cosine similarity of every view's condition image (surfd_amd.render.condition_image ->
preprocess.masked_crops -> clip_image_tensor, the image driver's own path) to the condition through
surfd_amd.clip_towers.ClipTowers; no CLIP weights ship here, so without ``--clip_weights`` the views are written, the script says
that the similarity was skipped, and exits 0.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfd_amd import meshprep, preprocess, render  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh", help="OBJ file")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default="outputs/render")
    ap.add_argument("--mode", default="perspective", choices=sorted(render.MODES))
    ap.add_argument("--elevation", type=float, default=20.0)
    ap.add_argument("--distance", type=float, default=2.6)
    ap.add_argument("--fov", type=float, default=40.0)
    ap.add_argument("--contours", action="store_true", help="also write line drawings (black on white)")
    ap.add_argument("--depth_jump", type=float, default=0.05)
    ap.add_argument("--crease", type=float, default=30.0, help="crease angle of the contours in degrees")
    ap.add_argument("--smooth", action="store_true", help="angle-weighted vertex normals instead of face normals")
    ap.add_argument("--clip_text", help="print every view's CLIP similarity to this prompt")
    ap.add_argument("--clip_image", help="print every view's CLIP similarity to this image (PNG)")
    ap.add_argument("--clip_weights", help="CLIP ViT-B/32 weights (TorchScript archive or state_dict); none ship here")
    ap.add_argument("--bpe_path", help="CLIP's BPE merges file (for --clip_text)")
    return ap.parse_args(argv)


def clip_similarities(a, views):
    """cosine similarity of every view to the condition, or None when the weights are not there"""
    if not a.clip_weights or not os.path.exists(a.clip_weights):
        print("CLIP similarity skipped: no weights file (--clip_weights); the views were written")
        return None
    from surfd_amd.clip_towers import ClipTowers, SimpleTokenizer
    dev = views["mask"].device
    towers = ClipTowers.from_file(a.clip_weights).to(dev)
    if a.clip_text:
        cond = towers.encode_text(SimpleTokenizer(a.bpe_path).tokenize([a.clip_text]).to(dev))
    else:
        img = render.read_png(a.clip_image)
        img = np.repeat(img[:, :, None], 3, 2) if img.ndim == 2 else img[:, :, :3]
        cond = towers.encode_image(preprocess.clip_image_tensor(img)[None].to(dev))
    crops = []
    for k in range(views["mask"].shape[0]):
        rgb, mask = render.condition_image(views, k)
        crops.append(preprocess.clip_image_tensor(preprocess.masked_crops(rgb, mask)[0]) if mask.any() else torch.zeros(3, 224, 224))
    emb = towers.encode_image(torch.stack(crops).to(dev))
    sim = torch.nn.functional.cosine_similarity(emb.float(), cond.float().expand_as(emb), dim=-1).cpu().tolist()
    for k, s in enumerate(sim):
        print(f"view {k}: cosine similarity {s:.4f}")
    return sim


def main(argv=None):
    a = parse(argv)
    v, f = meshprep.read_mesh(a.mesh)
    views = render.render_mesh(v.cuda(), f.cuda(), n_views=a.views, size=a.size, elevation_deg=a.elevation, distance=a.distance, mode=a.mode,
                               fov_deg=a.fov, smooth=a.smooth, contours=a.contours, depth_jump=a.depth_jump, crease_deg=a.crease)
    paths = render.save_views(a.out, os.path.splitext(os.path.basename(a.mesh))[0], views)
    covered = views["mask"].flatten(1).float().mean(1).cpu().tolist()
    print(f"{a.mesh}: {v.shape[0]} vertices, {f.shape[0]} faces -> {len(paths)} images in {a.out}; coverage per view "
          + " ".join(f"{c:.3f}" for c in covered) + f"; dropped triangles {views['dropped'].cpu().tolist()}")
    if a.clip_text or a.clip_image:
        clip_similarities(a, views)
    return paths


if __name__ == "__main__":
    main()
