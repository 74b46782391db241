#!/usr/bin/env python3
"""Meshes -> training items of the auto-encoder on the MI355X path: the counterpart of the reference's
AutoEncoder/encdec/preprocess_udfs.py (PrepareOneUDF, lines 118-151).

    python examples/preprocess_udfs.py --output_dir out/ chair.obj meshes/ [more OBJ files or directories]
    python examples/preprocess_udfs.py --num_surface_points 20000 --num_queries_per_std 5000 4000 500 500 --output_dir out/ a.obj

One ``<name>.npz`` per mesh with the reference's keys and dtypes: ``vertices`` [V, 3] float32, ``triangles`` [F, 3] int64,
``pcd`` [100 000, 3] float32 (a uniform surface cloud), ``coords`` [500 000, 3] float32 (queries around a second surface cloud
at sigma 0.003 / 0.01 / 0.1 plus uniform ones), ``labels`` [500 000] float32 (the UDF clipped to 0.1) and ``gradients``
[500 000, 3] float32.  The defaults are the reference's (100 000 surface points, 250 000 / 200 000 / 25 000 / 25 000 queries).
The files are inputs of examples/reconstruct.py.  Meshes are taken as already normalised to [-1, 1]^3 (the reference's separate
normalized_obj.py); a mesh with a vertex outside gets a warning.  The random numbers come from the GPU's global RNG, seeded
with ``--seed`` before every mesh.

    python examples/preprocess_udfs.py --signed --output_dir out/ closed.obj

``--signed`` writes the signed items of the reference's compute_sdf_from_mesh (AutoEncoder/utils.py:317-363) instead: ``labels``
is the signed distance clipped to +-0.1, negative inside, ``gradients`` carries its sign, and ``--num_queries_on_surface``
(10 000) points of the surface with label 0 and gradient 0 come first in ``coords``.  The sign is the parity of the mesh's
crossings along +z from the query and means something for a closed mesh only; ``--signed --sign winding`` takes it from the
generalized winding number instead (surfd_amd/winding.py: |w| >= 1/2 is inside), which survives small holes and needs
consistently oriented faces.  ``--orient`` gives them that first (surfd_amd/meshtopo.py: every manifold patch consistent, closed
patches outward; a patch that cannot be oriented stops the run) and ``--orient --weld`` takes the topology from the mesh with
coincident vertices welded, which is what dataset meshes that arrive as unwelded soups of mixed orientation need.  The written
``vertices`` / ``triangles`` stay the file's.  The same random numbers are drawn either way.  Without the flags nothing changes.

``--accel bvh`` searches the mesh through the box hierarchy of csrc/meshbvh.hip instead of its tiles: the files are the same
bytes.  The rays behind the sign of ``--signed`` go 4 to 24 times faster; the closest-point search does not yet (DESIGN.md
section 8.11 has the measurements).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfd_amd import meshprep  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inputs", nargs="+", help="OBJ files, or directories holding them")
    ap.add_argument("--output_dir", default="outputs/udfs")
    ap.add_argument("--num_surface_points", type=int, default=100_000)
    ap.add_argument("--num_queries_per_std", type=int, nargs=4, default=[250_000, 200_000, 25_000, 25_000],
                    metavar=("N_0.003", "N_0.01", "N_0.1", "N_UNIFORM"))
    ap.add_argument("--max_dist", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--signed", action="store_true", help="signed distances (negative inside) instead of unsigned ones; closed meshes only")
    ap.add_argument("--sign", choices=("parity", "winding"), default="parity",
                    help="with --signed: inside / outside by crossing parity (closed meshes) or by winding number (meshes with holes)")
    ap.add_argument("--orient", action="store_true",
                    help="with --signed --sign winding: give the faces a consistent, outward winding first (surfd_amd/meshtopo.py)")
    ap.add_argument("--weld", action="store_true",
                    help="with --orient: take the topology from the mesh with coincident vertices welded (for soups whose faces share no indices)")
    ap.add_argument("--num_queries_on_surface", type=int, default=10_000, help="with --signed: on-surface queries put in front")
    ap.add_argument("--accel", choices=("tiles", "bvh"), default="tiles",
                    help="how the mesh is searched: its tiles, or the box hierarchy (the same bytes; faster for the rays of --signed)")
    ap.add_argument("--winding_accel", choices=("exact", "bvh"), default="exact",
                    help="with --signed --sign winding: the exact sum over all faces, or the fast approximation (far parts of the mesh as dipoles)")
    ap.add_argument("--winding_beta", type=float, default=2.0, metavar="B",
                    help="--winding_accel bvh: a part of the mesh is approximated from B times its radius on (>= 1; larger is closer to exact)")
    return ap.parse_args(argv)


def winding_sdf_from_mesh(vs, ts, a, orient):
    """meshprep.compute_sdf_from_mesh(sign="winding") with the winding numbers of a WindingScene of the driver's own (the fast
    path): the same steps and the same random numbers in the same order"""
    from surfd_amd.winding import WindingScene
    cloud = meshprep.sample_points_uniformly(vs, ts, a.num_surface_points)
    queries = meshprep.sample_points_around_pcd(cloud, [0.003, 0.01, 0.1], list(a.num_queries_per_std), (-1.0, 1.0), vs.device)
    scene = WindingScene(vs, ts, orient=orient, accel=a.winding_accel, beta=a.winding_beta)
    sdf, gradients = meshprep.compute_sdf_and_gradients(scene, None, queries, sign="winding")
    on_surface = meshprep.sample_points_uniformly(vs, ts, a.num_queries_on_surface)
    n = a.num_queries_on_surface
    return (torch.cat([on_surface, queries]), torch.cat([sdf.new_zeros(n), sdf.clamp(-a.max_dist, a.max_dist)]),
            torch.cat([gradients.new_zeros(n, 3), gradients]))


def list_inputs(inputs):
    files = []
    for p in inputs:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith(".obj")]
        else:
            files.append(p)
    return files


def prepare_one(path, a):
    v, t = meshprep.read_mesh(path)
    if len(t) == 0:
        raise SystemExit(f"{path}: no faces")
    if float(v.abs().max()) > 1.0:
        print(f"warning: {path} has vertices outside [-1, 1]^3 (max |coordinate| {float(v.abs().max()):.4g}); queries are clipped "
              "to that cube, normalise the mesh first", file=sys.stderr)
    vd, td = v.cuda(), t.cuda()
    pcd = meshprep.sample_points_uniformly(vd, td, a.num_surface_points)                       # preprocess_udfs.py:126-127
    if a.signed:
        extra = {"accel": a.accel} if a.accel != "tiles" else {}
        vs, ts = vd, td
        if a.orient:
            from surfd_amd import meshtopo
            if a.weld:                                         # the sign comes from the welded mesh: the same surface, shared indices
                vs, ts, _ = meshtopo.weld_vertices(vd, td)
            extra["orient"] = "outward"
        if a.winding_accel != "exact":
            coords, labels, gradients = winding_sdf_from_mesh(vs, ts, a, extra.get("orient", False))
        else:
            coords, labels, gradients = meshprep.compute_sdf_from_mesh(vs, ts, num_surface_points=a.num_surface_points,
                                                                       num_queries_on_surface=a.num_queries_on_surface,
                                                                       num_queries_per_std=list(a.num_queries_per_std), max_dist=a.max_dist,
                                                                       sign=a.sign, **extra)
    else:
        coords, labels, gradients = meshprep.compute_udf_from_mesh(vd, td, num_surface_points=a.num_surface_points,
                                                                   num_queries_per_std=list(a.num_queries_per_std), max_dist=a.max_dist,
                                                                   **({"accel": a.accel} if a.accel != "tiles" else {}))
    return dict(vertices=v.numpy(), triangles=t.numpy(), pcd=pcd.cpu().numpy(), coords=coords.cpu().numpy(),
                labels=labels.cpu().numpy(), gradients=gradients.cpu().numpy())


def run(a):
    files = list_inputs(a.inputs)
    if not files:
        raise SystemExit("no input meshes")
    names = [os.path.splitext(os.path.basename(f))[0] for f in files]
    if len(set(names)) != len(names):
        raise SystemExit(f"item ids must be unique: {names}")
    if a.sign != "parity" and not a.signed:
        raise SystemExit("--sign chooses the sign of --signed items: it needs --signed")
    if a.orient and a.sign != "winding":
        raise SystemExit("--orient re-orients the faces for the winding number: it needs --signed --sign winding")
    if a.winding_accel != "exact" and a.sign != "winding":
        raise SystemExit("--winding_accel chooses how the winding number is summed: it needs --signed --sign winding")
    if not a.winding_beta >= 1.0:
        raise SystemExit(f"--winding_beta must be a number >= 1 (or inf), got {a.winding_beta}")
    if a.weld and not a.orient:
        raise SystemExit("--weld welds the mesh whose topology --orient uses: it needs --orient")
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_udfs.py runs on the GPU (no CPU fallback)")
    os.makedirs(a.output_dir, exist_ok=True)
    written = []
    for path, name in zip(files, names):
        torch.manual_seed(a.seed)
        item = prepare_one(path, a)
        out = os.path.join(a.output_dir, name + ".npz")
        np.savez(out, **item)
        written.append(out)
        print(f"{out}: {len(item['triangles'])} triangles, pcd {item['pcd'].shape[0]}, coords {item['coords'].shape[0]}, "
              f"mean label {float(item['labels'].mean()):.5f}")
    return written


def main(argv=None):
    return run(parse(argv))


if __name__ == "__main__":
    main()
