#!/usr/bin/env python3
"""Point clouds -> latents -> meshes on the MI355X path: the counterpart of the reference's
AutoEncoder/encdec/export_meshes.py (how a trained auto-encoder checkpoint is checked).

    python examples/reconstruct.py --ae_dir ae.pt --output_dir out/ cloud_0.npz cloud_1.npy [more files or directories]
    python examples/reconstruct.py --ae_dir ae.pt --latents_only --output_dir out/ clouds/      # -> out/latents.npz
    python examples/reconstruct.py --synthetic --resolution 64 --output_dir out/                 # smoke run, no trained weights

Inputs are point clouds: ``.npz`` files with the reference dataset's ``pcd`` key (AutoEncoder/data/dataset.py:82-83, written
by preprocess_udfs.py:128-151) or ``.npy`` arrays [N, 3]; the item id is the file name without its extension.  As in
export_meshes.py:55-100: the encoder and the decoder come from one checkpoint (``ckpt["encoder"]``, ``ckpt["decoder"]``; the
latent size is read from ``conv_5.weight``), every cloud is resampled to ``--num_points_pcd`` points with
random_point_sampling on the global RNG (seeded with ``--seed``), encoded by Dgcnn, and its UDF is meshed with
get_mesh_from_udf (or, with ``--watertight``, the level-set mesher).  The mesh is written as extracted, with no smoothing and
no component filtering (export_meshes.py:115-151).  ``--latents_only`` skips meshing and writes ``latents.npz`` (item id ->
latent), the data-export use (training_loop_single.py:107-112,190-194).  ``--synthetic`` writes a synthetic checkpoint holding
both encoder and decoder (surfd_amd.synth) and, when no input is given, two synthetic clouds.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from surfd_amd import meshproc, synth  # noqa: E402
from surfd_amd.cbndec import CbnDecoder, CoordsEncoder, make_udf_func  # noqa: E402
from surfd_amd.dgcnn import Dgcnn, random_point_sampling  # noqa: E402
from surfd_amd.meshudf import get_mesh_from_udf, get_watertight_mesh  # noqa: E402
from surfd_amd.rangeguard import run_guarded  # noqa: E402
from surfd_amd.spec import DecoderConfig  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("inputs", nargs="*", help=".npz (key 'pcd') / .npy [N,3] point clouds, or directories holding them")
    ap.add_argument("--ae_dir", help="auto-encoder checkpoint ({'encoder': state_dict, 'decoder': state_dict, ...})")
    ap.add_argument("--num_points_pcd", type=int, default=10000)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--watertight", action="store_true")
    ap.add_argument("--device_mc", action="store_true", help="--watertight: mesh the grid on the GPU (same mesh; the grid is not copied to the host)")
    ap.add_argument("--simplify_cells", type=int, default=None, metavar="K",
                    help="make the mesh smaller on the GPU before it is written: vertex clustering on a grid of K cells along the largest extent, "
                         "one quadric representative per occupied cell (surfd_amd.meshsimplify); with --watertight it needs --device_mc, open "
                         "meshes are then cleaned on the GPU too (device_clean: the same mesh)")
    ap.add_argument("--simplify_faces", type=int, default=None, metavar="N",
                    help="make the mesh smaller on the GPU before it is written: edge collapses down to N faces, borders kept, sheets not glued "
                         "(surfd_amd.meshsimplify.simplify_quadric_decimation); the same rules as --simplify_cells, and not together with it")
    ap.add_argument("--fill_holes", type=int, default=None, metavar="N",
                    help="close every border loop of up to N edges (3 .. 1024) on the GPU by its minimum-area triangulation before the mesh is "
                         "simplified, remeshed or written (surfd_amd.meshfill.fill_holes); the same rules as --simplify_cells")
    ap.add_argument("--remesh_edge", type=float, default=None, metavar="L",
                    help="remesh on the GPU before the mesh is written: triangles of roughly one size, edges of length L, vertices of valence 6 "
                         "(surfd_amd.meshremesh.remesh_isotropic); after --simplify_cells / --simplify_faces where given, the same rules as they")
    ap.add_argument("--remesh_edge_mean", type=float, default=None, metavar="K",
                    help="the same with L = K times the mean edge length of the mesh; not together with --remesh_edge (open meshes: the mesh is "
                         "remeshed as get_mesh_from_udf returns it, after the border smoothing, where --remesh_edge alone remeshes before it)")
    ap.add_argument("--remesh_iterations", type=int, default=5, metavar="N", help="--remesh_edge / --remesh_edge_mean: iterations (default 5)")
    ap.add_argument("--remesh_project", action="store_true",
                    help="--remesh_edge / --remesh_edge_mean: put the moved vertices back onto the mesh as it was before, after every iteration "
                         "(open meshes: remeshed as get_mesh_from_udf returns them, as with --remesh_edge_mean)")
    ap.add_argument("--batch", type=int, default=1, help="clouds per encoder call (export_meshes.py:75 uses 1)")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--output_dir", default="outputs/reconstruct")
    ap.add_argument("--latents_only", action="store_true", help="write latents.npz and skip meshing")
    ap.add_argument("--synthetic", action="store_true", help="create a synthetic checkpoint under --output_dir and use it")
    ap.add_argument("--size_latent", type=int, default=32, help="latent size of the --synthetic checkpoint")
    ap.add_argument("--metrics", action="store_true",
                    help="for inputs that carry 'vertices' / 'triangles' (examples/preprocess_udfs.py): write metrics.json")
    ap.add_argument("--accel", choices=("tiles", "bvh"), default="tiles",
                    help="--metrics: how mesh_distance searches the meshes: their tiles, or the box hierarchy of csrc/meshbvh.hip "
                         "(the same numbers; not faster yet for closest points: DESIGN.md section 8.11)")
    ap.add_argument("--mesh_quality", action="store_true",
                    help="--metrics: also record self_intersecting_faces, the share of the reconstruction's faces that pass through another, and "
                         "triangle_quality (edge lengths, smallest angles, valences; with --remesh_edge / --remesh_edge_mean before and after)")
    ap.add_argument("--topology", action="store_true",
                    help="--metrics: also record the reconstruction's topology (surfd_amd.meshtopo): pieces, holes, manifoldness, orientation")
    ap.add_argument("--preview", type=int, default=0, metavar="N",
                    help="also write N orbit views (shaded / depth / normal PNGs, surfd_amd.render) of every mesh; 0 = none")
    a = ap.parse_args(argv)
    if a.simplify_cells is not None and a.watertight and not a.device_mc:
        ap.error("--simplify_cells works on the device mesh: add --device_mc")
    if a.simplify_faces is not None and a.simplify_cells is not None:
        ap.error("--simplify_faces and --simplify_cells exclude each other")
    if a.simplify_faces is not None and a.watertight and not a.device_mc:
        ap.error("--simplify_faces works on the device mesh: add --device_mc")
    if a.simplify_faces is not None and a.simplify_faces < 0:
        ap.error("--simplify_faces must not be negative")
    if a.fill_holes is not None and a.watertight and not a.device_mc:
        ap.error("--fill_holes works on the device mesh: add --device_mc")
    if a.fill_holes is not None and not 3 <= a.fill_holes <= 1024:
        ap.error("--fill_holes must lie in [3, 1024]")
    remesh = a.remesh_edge is not None or a.remesh_edge_mean is not None
    if a.remesh_edge is not None and a.remesh_edge_mean is not None:
        ap.error("--remesh_edge and --remesh_edge_mean exclude each other")
    if remesh and a.watertight and not a.device_mc:
        ap.error("--remesh_edge works on the device mesh: add --device_mc")
    asked = a.remesh_edge if a.remesh_edge is not None else a.remesh_edge_mean
    if (remesh and not 0 < asked < float("inf")) or a.remesh_iterations < 0:
        ap.error("--remesh_edge / --remesh_edge_mean must be positive and finite, --remesh_iterations not negative")
    if (a.remesh_project or a.remesh_iterations != 5) and not remesh:
        ap.error("--remesh_iterations and --remesh_project go with --remesh_edge or --remesh_edge_mean")
    return a


def remesh_in_call(a):
    """the arguments of get_mesh_from_udf for --remesh_edge L alone: the call remeshes before it smooths the borders.  K times the
    mean edge length and the projection need the mesh itself: the driver remeshes what the call returns (remesh_on_device)"""
    if getattr(a, "remesh_edge", None) is None or getattr(a, "remesh_project", False):
        return {}
    return {"remesh_edge": a.remesh_edge, "remesh_iterations": a.remesh_iterations}


def remesh_on_device(a, verts, faces):
    """--remesh_edge / --remesh_edge_mean on a device mesh (float64 or float32 vertices, int64 faces); the mesh itself without them"""
    if (getattr(a, "remesh_edge", None) is None and getattr(a, "remesh_edge_mean", None) is None) or not len(faces):
        return verts, faces
    from surfd_amd.meshremesh import mean_edge_length, remesh_isotropic
    L = a.remesh_edge if a.remesh_edge is not None else a.remesh_edge_mean * mean_edge_length(verts, faces)
    ov, of = remesh_isotropic(verts, faces, L, iterations=a.remesh_iterations, project=a.remesh_project)
    return ov.to(verts.dtype), of


def synthetic_checkpoint(out_dir, size_latent):
    """encoder + decoder in the layout of the reference's auto-encoder checkpoint.  The untrained decoder's logit stays below
    the level the meshers extract at for the encoder's latents; its output bias is raised by 1 so that the field has a surface."""
    path = os.path.join(out_dir, "ae_synthetic.pt")
    dec = synth.synth_decoder_state_dict(DecoderConfig(latent_dim=size_latent))
    dec["decoder.fc_out.bias"] = dec["decoder.fc_out.bias"] + 1.0
    torch.save({"epoch": 0, "encoder": synth.synth_dgcnn_state_dict(size_latent), "decoder": dec}, path)
    return path


def synthetic_clouds(out_dir, count=2, n=12000):
    """points near a torus (R 0.5, r 0.15 + 0.05 i), written in the dataset's npz layout"""
    paths = []
    g = torch.Generator().manual_seed(7)
    for i in range(count):
        u, v = torch.rand(n, generator=g) * 2 * np.pi, torch.rand(n, generator=g) * 2 * np.pi
        r = 0.15 + 0.05 * i
        pcd = torch.stack([(0.5 + r * torch.cos(v)) * torch.cos(u), r * torch.sin(v), (0.5 + r * torch.cos(v)) * torch.sin(u)], 1)
        path = os.path.join(out_dir, f"synthetic_{i}.npz")
        np.savez(path, pcd=pcd.numpy().astype(np.float32))
        paths.append(path)
    return paths


def list_inputs(inputs):
    files = []
    for p in inputs:
        if os.path.isdir(p):
            files += [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.endswith((".npz", ".npy"))]
        else:
            files.append(p)
    return files


def load_cloud(path) -> torch.Tensor:
    if path.endswith(".npz"):
        with np.load(path) as z:
            if "pcd" not in z.files:
                raise SystemExit(f"{path}: no 'pcd' array (keys: {z.files})")
            pcd = z["pcd"]
    else:
        pcd = np.load(path)
    if pcd.ndim != 2 or pcd.shape[1] != 3:
        raise SystemExit(f"{path}: expected a point cloud [N, 3], got {pcd.shape}")
    return torch.from_numpy(np.ascontiguousarray(pcd, dtype=np.float32))


def load_models(ae_dir):
    ckpt = torch.load(ae_dir, map_location="cpu")
    for key in ("encoder", "decoder"):
        if key not in ckpt:
            raise SystemExit(f"{ae_dir}: no '{key}' state dict (keys: {list(ckpt)})")
    size_latent = int(ckpt["encoder"]["conv_5.weight"].shape[0])
    encoder = Dgcnn(size_latent)
    encoder.load_state_dict(ckpt["encoder"], strict=True)
    encoder = encoder.cuda().eval()
    dec_latent = next((v.shape[1] for k, v in ckpt["decoder"].items() if k.endswith("conv_gamma.weight")), None)
    if dec_latent is not None and dec_latent != size_latent:
        raise SystemExit(f"{ae_dir}: the encoder makes {size_latent}-d latents, the decoder takes {dec_latent}-d ones")
    decoder = CbnDecoder(CoordsEncoder().out_dim, size_latent, 512, 5)
    decoder.load_state_dict(ckpt["decoder"], strict=True)
    return encoder, decoder.cuda().eval(), size_latent


def triangle_quality_of(a, verts, faces, shape_mesh):
    """--metrics --mesh_quality: surfd_amd.meshremesh.triangle_quality of the mesh written, and with --remesh_edge /
    --remesh_edge_mean also of the mesh the same call gives without them (it is meshed once more for that), both against the
    edge length the remeshing aimed at"""
    import argparse
    from surfd_amd.meshremesh import mean_edge_length, triangle_quality

    def on_device(v, t):
        return (torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64)).cuda(), torch.as_tensor(np.ascontiguousarray(t, dtype=np.int64)).reshape(-1, 3).cuda())
    if a.remesh_edge is None and a.remesh_edge_mean is None:
        return {"triangle_quality": triangle_quality(*on_device(verts, faces))}
    plain = argparse.Namespace(**dict(vars(a), remesh_edge=None, remesh_edge_mean=None))
    bv, bt = on_device(*shape_mesh(plain))
    L = a.remesh_edge if a.remesh_edge is not None else a.remesh_edge_mean * mean_edge_length(bv, bt)
    return {"remesh_edge_length": L, "triangle_quality_before_remesh": triangle_quality(bv, bt, L),
            "triangle_quality": triangle_quality(*on_device(verts, faces), L)}


def item_metrics(path, verts, faces, field, seed, mesh_quality=False, accel="tiles", topology=False, hole_filling=None):
    """what --metrics records for one item, or None where the input carries no mesh: mesh_distance between the reconstruction
    and the original; the IoU of their surface voxels on a 64^3 grid over [-1, 1]^3 (voxel_iou_surface_64); the normal
    consistency of 16 Ki = 16 384 surface points per mesh with their face normals, unsigned (normal_consistency_16: the number
    counts samples, no neighbourhood size enters); and, where the file has 'coords' / 'labels', the mean absolute error of the
    decoder's UDF at those queries.  ``mesh_quality`` adds self_intersecting_faces: the share of the reconstruction's faces with
    area that pass through or touch another of its faces beyond what neighbours share (surfd_amd.meshintersect).  ``topology``
    adds topology: the numbers of surfd_amd.meshtopo.MeshTopology.summary() for the reconstruction without its per-patch list
    (edges by class, Euler characteristic, components, border loops, closed, edge_manifold, orientable, ...) and, with
    ``hole_filling`` (the counts of --fill_holes: loops_filled, caps, loops_too_long, irregular_border_edges, ...), those counts as
    hole_filling and the lengths of the border loops that are left as border_loop_sizes (surfd_amd.meshfill.hole_sizes).  ``accel``:
    how mesh_distance searches the two meshes ("tiles" or "bvh": the same numbers)"""
    from surfd_amd import meshprep
    if not path.endswith(".npz"):
        return None
    with np.load(path) as z:
        if "vertices" not in z.files or "triangles" not in z.files:
            return None
        ov, ot = torch.from_numpy(z["vertices"].astype(np.float32)).cuda(), torch.from_numpy(z["triangles"].astype(np.int64)).cuda()
        coords = torch.from_numpy(z["coords"].astype(np.float32)).cuda() if "coords" in z.files and "labels" in z.files else None
        labels = torch.from_numpy(z["labels"].astype(np.float32)).cuda() if coords is not None else None
    out = {"vertices": int(len(verts)), "faces": int(len(faces))}
    if len(faces):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rv, rt = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).cuda()
        d = meshprep.mesh_distance(rv, rt, ov, ot, generator=g, **({"accel": accel} if accel != "tiles" else {}))
        out.update(reconstruction_to_original=d["d12"], original_to_reconstruction=d["d21"], mesh_distance=d["sum"])
        from surfd_amd import voxelize
        out["voxel_iou_surface_64"] = float(voxelize.voxel_iou(voxelize.voxelize_surface(rv, rt, 64), voxelize.voxelize_surface(ov, ot, 64)))
        from surfd_amd import cloudmetrics
        rp, rn, _ = meshprep.sample_points_with_normals(rv, rt, 16384, generator=g)
        op, on, _ = meshprep.sample_points_with_normals(ov, ot, 16384, generator=g)
        out["normal_consistency_16"] = float(cloudmetrics.normal_consistency(rp[None], rn[None], op[None], on[None])["nc"])
        if mesh_quality:
            from surfd_amd import meshintersect
            out["self_intersecting_faces"] = meshintersect.self_intersections(rv, rt, return_pairs=False)["fraction"]
        if topology:
            from surfd_amd import meshtopo
            out["topology"] = {k: v for k, v in meshtopo.MeshTopology(rt, len(verts)).summary().items() if k != "patches"}
            if hole_filling is not None:
                from surfd_amd import meshfill
                out["topology"]["hole_filling"] = dict(hole_filling)
                out["topology"]["border_loop_sizes"] = meshfill.hole_sizes(rv, rt)
    if coords is not None:
        pred = torch.cat([field(coords[i:i + 2 ** 16]) for i in range(0, len(coords), 2 ** 16)])
        out["udf_mean_abs_error"] = float((pred.reshape(-1) - labels).abs().double().mean())
    return out


def main(argv=None):
    return run(parse(argv))


def run(a):
    if a.accel != "tiles" and not a.metrics:
        raise SystemExit("--accel chooses how --metrics measures: it needs --metrics")
    if a.mesh_quality and not a.metrics:
        raise SystemExit("--mesh_quality adds to metrics.json: it needs --metrics")
    if a.topology and not a.metrics:
        raise SystemExit("--topology adds to metrics.json: it needs --metrics")
    os.makedirs(a.output_dir, exist_ok=True)
    inputs = list(a.inputs)
    if a.synthetic:
        a.ae_dir = synthetic_checkpoint(a.output_dir, a.size_latent)
        if not inputs:
            inputs = synthetic_clouds(a.output_dir)
    if not a.ae_dir:
        raise SystemExit("--ae_dir is required (or --synthetic)")
    files = list_inputs(inputs)
    if not files:
        raise SystemExit("no input point clouds")
    encoder, decoder, size_latent = load_models(a.ae_dir)
    torch.manual_seed(a.seed)

    ids, latents = [], []
    for b0 in range(0, len(files), a.batch):
        chunk = files[b0:b0 + a.batch]
        pcds = torch.stack([random_point_sampling(load_cloud(f).cuda(), a.num_points_pcd) for f in chunk])   # as export_meshes.py:79-83
        latents.append(encoder(pcds))
        ids += [os.path.splitext(os.path.basename(f))[0] for f in chunk]
    latents = torch.cat(latents)
    if len(set(ids)) != len(ids):
        raise SystemExit(f"item ids must be unique: {ids}")
    if a.latents_only:
        path = os.path.join(a.output_dir, "latents.npz")
        np.savez(path, **{i: latents[k].cpu().numpy() for k, i in enumerate(ids)})
        print(f"{path}: {len(ids)} latents of size {size_latent}")
        return latents, [path]

    decoder.bind_latents(latents)
    written = []
    metrics = {}
    for k, item in enumerate(ids):
        field = make_udf_func(decoder, latents[k], sample=k)
        filled = {}                                          # the counts of --fill_holes for this item

        def shape_mesh(a=a):
            if a.watertight and a.device_mc:
                v, t = get_watertight_mesh(field, a.resolution, max_batch=2 ** 16, device=True)
                if getattr(a, "fill_holes", None) is not None and len(t):
                    from surfd_amd.meshfill import fill_holes
                    t, counts = fill_holes(v, t, max_edges=a.fill_holes, return_stats=True)
                    filled.update(counts)
                if a.simplify_cells is not None and len(t):
                    from surfd_amd.meshsimplify import simplify_vertex_clustering
                    v, t = simplify_vertex_clustering(v, t, cells=a.simplify_cells)
                if a.simplify_faces is not None and len(t):
                    from surfd_amd.meshsimplify import simplify_quadric_decimation
                    v, t = simplify_quadric_decimation(v, t, a.simplify_faces)
                v, t = remesh_on_device(a, v, t)
                return v.cpu().numpy(), t.cpu().numpy()
            if a.watertight:
                return get_watertight_mesh(field, a.resolution, max_batch=2 ** 16)
            fill = getattr(a, "fill_holes", None)
            v, t, *counts = get_mesh_from_udf(field, coords_range=(-1, 1), max_dist=0.1, N=a.resolution, max_batch=2 ** 16, differentiable=False,
                                     device_clean=a.simplify_cells is not None or a.simplify_faces is not None or a.remesh_edge is not None or
                                     a.remesh_edge_mean is not None or fill is not None,
                                     simplify_cells=a.simplify_cells, simplify_faces=a.simplify_faces,
                                     **({"fill_holes": fill, "return_fill_stats": True} if fill is not None else {}),
                                     **remesh_in_call(a))
            if counts:
                filled.update(counts[0])
            if not remesh_in_call(a):
                v, t = remesh_on_device(a, v, t)
            return v.cpu().numpy(), t.cpu().numpy()

        (verts, faces), _ = run_guarded(f"{item} (decoder grids)", shape_mesh, decoder.saturation_count,
                                        lambda: decoder.set_precision("fp32"))
        path = os.path.join(a.output_dir, f"{item}_{'watertight' if a.watertight else 'meshudf'}.obj")
        meshproc.write_obj(path, verts, faces)
        written.append(path)
        print(f"{path}: {len(verts)} vertices, {len(faces)} faces")
        if a.preview > 0:
            from surfd_amd import render
            views = render.render_mesh(torch.as_tensor(np.ascontiguousarray(verts, dtype=np.float32)).cuda(),
                                       torch.as_tensor(np.ascontiguousarray(faces, dtype=np.int64)).reshape(-1, 3).cuda(), n_views=a.preview, size=512)
            written += render.save_views(a.output_dir, os.path.splitext(os.path.basename(path))[0], views)
        if a.metrics:
            m = item_metrics(files[k], verts, faces, field, a.seed, a.mesh_quality, a.accel, a.topology, filled if a.fill_holes is not None else None)
            if m is not None and a.mesh_quality and len(faces):
                m.update(triangle_quality_of(a, verts, faces, shape_mesh))
            if m is not None:
                metrics[item] = m
    if a.metrics:
        import json
        path = os.path.join(a.output_dir, "metrics.json")
        with open(path, "w") as f:
            json.dump(metrics, f, indent=1)
        written.append(path)
        print(f"{path}: {len(metrics)} items")
    return latents, written


if __name__ == "__main__":
    main()
