#!/usr/bin/env python3
"""Scores generated shapes against a held-out set, or reconstructions against their originals, on the MI355X path
(surfd_amd/cloudmetrics.py).  The reference ships no evaluation code; the protocol is that of Achlioptas et al. 2018 as used in
PointFlow: clouds of ``--num_points`` points, Chamfer distance = sum of the two directed means of squared nearest-neighbour
distances.

    python examples/evaluate.py --generated outputs/meshes --reference data/heldout --output metrics.json
    python examples/evaluate.py --generated outputs/rec --reference data/items --paired --output pairs.json

Each directory holds ``.obj`` meshes (sampled uniformly on their surface) and / or ``.npz`` files with a ``pcd`` or ``points``
array as examples/preprocess_udfs.py writes them (subsampled at random without replacement; a smaller cloud is an error).  All
random numbers come from one CPU generator seeded with ``--seed``, used file by file in sorted order, the generated directory
first.  Default: the set metrics MMD-CD, COV-CD and 1-NNA-CD in one JSON with the counts and the options used.  ``--paired``:
files are matched by stem and every pair gets ``cd``, ``fscore``, ``precision``, ``recall`` (generated = prediction), plus their
means.  The earth mover's distance is not computed.

``--sampling even`` replaces the random draws by clouds that cover their shape evenly: an ``.obj`` item is sampled with
``meshprep.sample_points_evenly`` (``--init_factor`` x ``--num_points`` uniform candidates, then farthest point sampling), an
``.npz`` cloud with more than ``--num_points`` points is reduced by farthest point sampling from its first point instead of a
random subset (surfd_amd/cloudsample.py).  The output JSON then records ``sampling`` and ``init_factor`` among its options;
the default, ``uniform``, is the behaviour described above and leaves the JSON as it was.

``--paired --voxel_iou R`` adds the volumetric IoU of every pair on an R^3 grid over ``--voxel_bounds`` (surfd_amd/voxelize.py):
``--voxel_mode surface`` (voxels the triangles touch), ``solid`` (parity fill | surface; each item's ``odd_columns`` is recorded,
0 for a closed mesh), ``winding`` (voxels whose centre has |generalized winding number| >= 1/2, surfd_amd/winding.py: the fill
for meshes with small holes, where ``solid`` leaks along every column through a hole; it needs consistently oriented faces) or
``points`` (voxels that hold a vertex of the mesh or a point of the .npz cloud, all of them, no subsampling).  Both items of a
pair are voxelised in ONE frame: with ``--normalize bbox`` / ``unit_sphere`` the transform of the
REFERENCE item (from its vertices or points) is applied to both.  ``.npz`` clouds are scored in ``points`` mode only; elsewhere
the pair is listed under ``skipped``.

``--paired --normal_consistency`` adds the normal consistency of every pair: normals are estimated on both final clouds (after
sampling and normalisation, so ``.obj`` and ``.npz`` items are treated alike, as a scan would be) from their ``--normals_k``
nearest neighbours (surfd_amd/cloudnormals.py), and every point's normal is compared with that of its nearest neighbour in the
other cloud: the mean of |<n, n'>| in both directions, averaged (cloudmetrics.normal_consistency; 1 = the same orientation
everywhere).  The JSON then records ``normal_consistency`` and ``normals_k`` among its options.

``--paired --self_intersections`` adds, for the GENERATED item of every pair, ``self_intersecting_faces`` (the share of its faces
with area that pass through another face of the same mesh), ``self_intersecting_pairs`` (how many pairs of faces do) and
``degenerate_faces`` (faces without area), plus their means (surfd_amd/meshintersect.py: exact integer predicates on the raw
file's vertices snapped to the finest lattice that holds them; touching and T-junctions count).  ``--paired --topology`` adds,
for the GENERATED item of every pair, ``topology``: the numbers of surfd_amd.meshtopo (edges by class, Euler characteristic,
components under the three connectivities, border loops and the largest, closed, edge_manifold, orientable,
consistently_oriented) on the file's own indices, and their means as ``topology_*``.  ``--paired --collisions`` adds
``colliding_faces``: the share of the generated item's faces that pass through or touch a face of the reference item, both in
the frame of the raw files, no normalisation.  Both need meshes: a pair with an ``.npz`` item where a mesh is needed is listed
under ``skipped``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfd_amd import cloudmetrics, cloudnormals, cloudsample, meshprep  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--generated", required=True, help="directory of .obj / .npz files")
    ap.add_argument("--reference", required=True, help="directory of .obj / .npz files")
    ap.add_argument("--paired", action="store_true", help="match files by stem and score every pair")
    ap.add_argument("--num_points", type=int, default=2048)
    ap.add_argument("--normalize", choices=("none", "unit_sphere", "bbox"), default="bbox")
    ap.add_argument("--f_threshold", type=float, default=0.01, help="distance threshold of the F-score (--paired)")
    ap.add_argument("--chunk", type=int, default=None, help="clouds per kernel launch (results do not depend on it)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sampling", choices=("uniform", "even"), default="uniform",
                    help="uniform: random surface samples / random subsets; even: farthest point sampling (see above)")
    ap.add_argument("--init_factor", type=int, default=5, help="--sampling even: uniform candidates per kept point of an .obj item")
    ap.add_argument("--voxel_iou", type=int, default=0, metavar="R", help="--paired: also score volumetric IoU on an R^3 grid (0 = off)")
    ap.add_argument("--voxel_bounds", type=float, nargs=2, default=(-1.0, 1.0), metavar=("LO", "HI"))
    ap.add_argument("--voxel_mode", choices=("surface", "solid", "winding", "points"), default="surface")
    ap.add_argument("--winding_accel", choices=("exact", "bvh"), default="exact",
                    help="--voxel_mode winding: the exact sum over all faces, or the fast approximation (far parts of the mesh as dipoles)")
    ap.add_argument("--winding_beta", type=float, default=2.0, metavar="B",
                    help="--winding_accel bvh: a part of the mesh is approximated from B times its radius on (>= 1; larger is closer to exact)")
    ap.add_argument("--normal_consistency", action="store_true", help="--paired: also score the normal consistency of every pair")
    ap.add_argument("--normals_k", type=int, default=16, metavar="K", help="--normal_consistency: neighbours per estimated normal (3 .. 64)")
    ap.add_argument("--self_intersections", action="store_true", help="--paired: also report the self-intersections of every generated mesh")
    ap.add_argument("--collisions", action="store_true", help="--paired: also report the faces of every generated mesh that meet its reference mesh")
    ap.add_argument("--topology", action="store_true", help="--paired: also report the topology of every generated mesh (pieces, holes, manifoldness)")
    ap.add_argument("--output", default="metrics.json")
    return ap.parse_args(argv)


def list_items(directory):
    """{stem: path} of the .obj / .npz files of a directory, sorted by stem"""
    if not os.path.isdir(directory):
        raise SystemExit(f"{directory} is not a directory")
    items = {}
    for f in sorted(os.listdir(directory)):
        stem, ext = os.path.splitext(f)
        if ext.lower() in (".obj", ".npz"):
            if stem in items:
                raise SystemExit(f"{directory}: item id '{stem}' appears twice")
            items[stem] = os.path.join(directory, f)
    if not items:
        raise SystemExit(f"{directory}: no .obj or .npz files")
    return dict(sorted(items.items()))


def load_cloud(path, num_points, generator, sampling="uniform", init_factor=5):
    """one file -> [num_points, 3] float32 on the CPU"""
    if path.lower().endswith(".obj"):
        v, t = meshprep.read_mesh(path)
        if len(t) == 0:
            raise SystemExit(f"{path}: no faces")
        if sampling == "even":
            return meshprep.sample_points_evenly(v, t, num_points, init_factor=init_factor, generator=generator)
        return meshprep.sample_points_uniformly(v, t, num_points, generator=generator)
    z = np.load(path)
    key = next((k for k in ("pcd", "points") if k in z.files), None)
    if key is None:
        raise SystemExit(f"{path}: neither 'pcd' nor 'points' inside")
    p = torch.from_numpy(np.asarray(z[key], dtype=np.float32)).reshape(-1, 3)
    if len(p) < num_points:
        raise SystemExit(f"{path}: {len(p)} points, fewer than --num_points {num_points}")
    if sampling == "even" and len(p) > num_points:
        if not bool(torch.isfinite(p).all()):
            raise SystemExit(f"{path}: the cloud contains NaN or Inf")
        return cloudsample.sample_farthest_points(p[None].contiguous().cuda(), num_points)[0][0].cpu()
    return p[torch.randperm(len(p), generator=generator)[:num_points]].contiguous()


def load_set(items, a, generator):
    x = torch.stack([load_cloud(p, a.num_points, generator, a.sampling, a.init_factor) for p in items.values()])
    if not bool(torch.isfinite(x).all()):
        raise SystemExit("a cloud contains NaN or Inf")
    return cloudmetrics.normalize_clouds(x, a.normalize).contiguous()


def load_geometry(path):
    """one file -> (points or vertices [N, 3] float32, faces [F, 3] or None) on the CPU, nothing sampled"""
    if path.lower().endswith(".obj"):
        v, t = meshprep.read_mesh(path)
        return torch.as_tensor(np.asarray(v, dtype=np.float32)).reshape(-1, 3), torch.as_tensor(np.asarray(t).astype(np.int32)).reshape(-1, 3)
    z = np.load(path)
    key = next((k for k in ("pcd", "points") if k in z.files), None)
    if key is None:
        raise SystemExit(f"{path}: neither 'pcd' nor 'points' inside")
    return torch.from_numpy(np.asarray(z[key], dtype=np.float32)).reshape(-1, 3), None


def reference_frame(x, mode):
    """(centre [3], radius) of cloudmetrics.normalize_clouds(x, mode), to be applied to both items of a pair"""
    if mode == "none":
        return torch.zeros(3), 1.0
    if mode == "unit_sphere":
        c = x.mean(0)
        r = float((x - c).norm(dim=-1).amax())
    else:
        lo, hi = x.amin(0), x.amax(0)
        c = (lo + hi) / 2
        r = float((hi - lo).amax()) / 2
    return c, (r if r > 0 else 1.0)


def voxel_scores(gen_items, ref_items, a):
    """-> (per-item dict, skipped ids) of --voxel_iou"""
    from surfd_amd import voxelize
    R, bounds = a.voxel_iou, tuple(a.voxel_bounds)
    items, skipped = {}, []
    for name in gen_items:
        (gv, gf), (rv, rf) = load_geometry(gen_items[name]), load_geometry(ref_items[name])
        if a.voxel_mode != "points" and (gf is None or rf is None or not len(gf) or not len(rf)):
            skipped.append(name)
            continue
        c, r = reference_frame(rv, a.normalize)
        entry, grids = {}, []
        for v, f, side in ((gv, gf, "generated"), (rv, rf, "reference")):
            v = ((v - c) / r).contiguous().cuda()
            if a.voxel_mode == "points":
                grids.append(voxelize.voxelize_points(v, R, bounds))
            elif a.voxel_mode == "surface":
                grids.append(voxelize.voxelize_surface(v, f.cuda(), R, bounds))
            elif a.voxel_mode == "winding":
                grids.append(voxelize.voxelize_winding(v, f.cuda(), R, bounds, accel=a.winding_accel, beta=a.winding_beta))
            else:
                grid, odd = voxelize.voxelize_solid(v, f.cuda(), R, bounds)
                grids.append(grid)
                entry[f"odd_columns_{side}"] = odd
        entry["voxel_iou"] = float(voxelize.voxel_iou(grids[0], grids[1]))
        items[name] = entry
    return items, skipped


def _mesh_on_device(path):
    v, f = load_geometry(path)
    if f is None or not len(f):
        return None
    return v.contiguous().cuda(), f.contiguous().cuda()


def intersection_scores(gen_items, ref_items, a):
    """-> (per-item dict, skipped ids) of --self_intersections and --collisions"""
    from surfd_amd import meshintersect
    items, skipped = {}, []
    for name in gen_items:
        gen = _mesh_on_device(gen_items[name])
        ref = _mesh_on_device(ref_items[name]) if a.collisions else None
        if gen is None or (a.collisions and ref is None):
            skipped.append(name)
            continue
        entry = {}
        if a.self_intersections:
            r = meshintersect.self_intersections(*gen, return_pairs=False)
            entry.update(self_intersecting_faces=r["fraction"], self_intersecting_pairs=r["count"], degenerate_faces=int(r["degenerate"].sum()))
        if a.collisions:
            entry["colliding_faces"] = meshintersect.mesh_intersections(*gen, *ref, return_pairs=False)["fraction"]
        items[name] = entry
    return items, skipped


def topology_scores(gen_items):
    """-> (per-item dict, skipped ids) of --topology: surfd_amd.meshtopo.MeshTopology.summary() of the generated mesh without its
    per-patch list, under the key ``topology``"""
    from surfd_amd import meshtopo
    items, skipped = {}, []
    for name in gen_items:
        gen = _mesh_on_device(gen_items[name])
        if gen is None:
            skipped.append(name)
            continue
        items[name] = {"topology": {k: v for k, v in meshtopo.MeshTopology(gen[1], gen[0].shape[0]).summary().items() if k != "patches"}}
    return items, skipped


def run(a):
    if a.topology and not a.paired:
        raise SystemExit("--topology describes the generated item of every pair: it needs --paired")
    if a.self_intersections and not a.paired:
        raise SystemExit("--self_intersections scores the generated item of every pair: it needs --paired")
    if a.collisions and not a.paired:
        raise SystemExit("--collisions scores pairs: it needs --paired")
    if a.voxel_iou and not a.paired:
        raise SystemExit("--voxel_iou scores pairs: it needs --paired")
    if a.winding_accel != "exact" and not (a.voxel_iou and a.voxel_mode == "winding"):
        raise SystemExit("--winding_accel chooses how the winding number is summed: it needs --voxel_iou R --voxel_mode winding")
    if not a.winding_beta >= 1.0:
        raise SystemExit(f"--winding_beta must be a number >= 1 (or inf), got {a.winding_beta}")
    if a.normal_consistency and not a.paired:
        raise SystemExit("--normal_consistency scores pairs: it needs --paired")
    if a.normal_consistency and not (cloudnormals.K_MIN <= a.normals_k <= min(cloudnormals.K_MAX, a.num_points)):
        raise SystemExit(f"--normals_k must lie in {cloudnormals.K_MIN} .. {cloudnormals.K_MAX} and not exceed --num_points")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py runs on the GPU (no CPU fallback)")
    if a.init_factor < 1:
        raise SystemExit("--init_factor must be at least 1")
    gen_items, ref_items = list_items(a.generated), list_items(a.reference)
    if a.paired:
        if list(gen_items) != list(ref_items):
            raise SystemExit(f"--paired needs the same item ids on both sides; unmatched: {sorted(set(gen_items) ^ set(ref_items))}")
    g = torch.Generator().manual_seed(a.seed)
    gen = load_set(gen_items, a, g).cuda()
    ref = load_set(ref_items, a, g).cuda()
    out = {"options": {"num_points": a.num_points, "normalize": a.normalize, "seed": a.seed, "paired": bool(a.paired)},
           "num_generated": len(gen_items), "num_reference": len(ref_items)}
    if a.sampling != "uniform":
        out["options"].update(sampling=a.sampling, init_factor=a.init_factor)
    if a.paired:
        out["options"]["f_threshold"] = a.f_threshold
        r = {k: v.cpu().tolist() for k, v in cloudmetrics.chamfer_distance(gen, ref, f_threshold=a.f_threshold).items()}
        keys = ("cd", "fscore", "precision", "recall")
        out["items"] = {name: {k: r[k][i] for k in keys} for i, name in enumerate(gen_items)}
        out["mean"] = {k: float(np.mean(r[k], dtype=np.float64)) for k in keys}
        if a.voxel_iou:
            out["options"].update(voxel_iou=a.voxel_iou, voxel_bounds=list(a.voxel_bounds), voxel_mode=a.voxel_mode)
            if a.winding_accel != "exact":
                out["options"].update(winding_accel=a.winding_accel, winding_beta=a.winding_beta)
            scores, skipped = voxel_scores(gen_items, ref_items, a)
            for name, s in scores.items():
                out["items"][name].update(s)
            if scores:
                out["mean"]["voxel_iou"] = float(np.mean([s["voxel_iou"] for s in scores.values()], dtype=np.float64))
            out["skipped"] = skipped
        if a.normal_consistency:
            out["options"].update(normal_consistency=True, normals_k=a.normals_k)
            n_gen, n_ref = cloudnormals.estimate_normals(gen, k=a.normals_k)[0], cloudnormals.estimate_normals(ref, k=a.normals_k)[0]
            nc = cloudmetrics.normal_consistency(gen, n_gen, ref, n_ref)["nc"].cpu().tolist()
            for i, name in enumerate(gen_items):
                out["items"][name]["normal_consistency"] = nc[i]
            out["mean"]["normal_consistency"] = float(np.mean(nc, dtype=np.float64))
        if a.self_intersections or a.collisions:
            out["options"].update({k: True for k in ("self_intersections", "collisions") if getattr(a, k)})
            scores, skipped = intersection_scores(gen_items, ref_items, a)
            for name, s in scores.items():
                out["items"][name].update(s)
            for k in ("self_intersecting_faces", "self_intersecting_pairs", "degenerate_faces", "colliding_faces"):
                if scores and k in next(iter(scores.values())):
                    out["mean"][k] = float(np.mean([s[k] for s in scores.values()], dtype=np.float64))
            out["skipped"] = sorted(set(out.get("skipped", [])) | set(skipped))
        if a.topology:
            out["options"]["topology"] = True
            scores, skipped = topology_scores(gen_items)
            for name, s in scores.items():
                out["items"][name].update(s)
            for k in ("components_vertex", "border_loops", "non_manifold_edges"):
                if scores:
                    out["mean"]["topology_" + k] = float(np.mean([s["topology"][k] for s in scores.values()], dtype=np.float64))
            if scores:
                out["mean"]["topology_closed"] = float(np.mean([s["topology"]["closed"] for s in scores.values()], dtype=np.float64))
            out["skipped"] = sorted(set(out.get("skipped", [])) | set(skipped))
    else:
        m = cloudmetrics.compute_all_metrics(gen, ref, chunk=a.chunk)
        out["metrics"] = {"mmd_cd": m["mmd_cd"], "cov_cd": m["cov_cd"], "1nna_cd": m["1nna_cd"]}
        out["detail"] = {k: m[k] for k in ("mmd_smp_cd", "1nna_cd_gen", "1nna_cd_ref")}
    os.makedirs(os.path.dirname(os.path.abspath(a.output)), exist_ok=True)
    with open(a.output, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out.get("metrics", out.get("mean"))))
    return out


def main(argv=None):
    return run(parse(argv))


if __name__ == "__main__":
    main()
