#!/usr/bin/env python3
"""Device-event timing of the mesh topology (surfd_amd.meshtopo, csrc/meshtopo.hip) after warm-up, on icospheres of 20 480,
81 920, 327 680 and 1 310 720 faces with a seeded 40 % of the faces turned and the face order shuffled, and on the strip of
100 000 triangles in a row (diameter 100 000: the worst case for path compression): build (sort + edges), each connectivity,
orientation, orientation with the outward pass, border loops and the exact weld of the mesh exploded into a soup; each the
median of repeated calls with events on one stream (the calls that read a count back include that sync).  Next to them the host
numpy time of the only counterparts the package has, meshproc.face_components and meshproc.border_edge_rows, on the same mesh
and the same box (wall clock, median).  No ratio is asserted anywhere: the numbers are recorded as measured.

    python tools/meshtopo_time.py [--out profiles/meshtopo_time.json] [--reps 10] [--levels 5 6 7 8]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import meshtopo_ref as MT  # noqa: E402
import raycast_ref as RR  # noqa: E402
from surfd_amd import meshproc  # noqa: E402
from surfd_amd.meshtopo import MeshTopology, weld_vertices  # noqa: E402


def icosphere(level):
    """raycast_ref.icosphere's surface with the midpoints found by sorting instead of a dict (level 8 has 1.3 million faces)"""
    v, f = RR.icosphere(0, 1.0)
    v = v.astype(np.float64)
    for _ in range(level):
        e = np.sort(np.stack([f, f[:, [1, 2, 0]]], 2).reshape(-1, 2), 1)
        uniq, inv = np.unique(e[:, 0] * len(v) + e[:, 1], return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        m = inv.reshape(-1, 3) + len(v)                                   # midpoints of (a b), (b c), (c a)
        v = np.concatenate([v, mid / np.linalg.norm(mid, axis=1, keepdims=True)])
        a, b, c, ab, bc, ca = f[:, 0], f[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]
        f = np.stack([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)], 1).reshape(-1, 3)
    return (v * 0.75).astype(np.float32), f.astype(np.int64)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def host_timed(fn, reps=3):
    times = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); times.append((time.perf_counter() - t) * 1e3)
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def fresh(topo, fn):
    """the call with the object's kept results dropped, so that every repeat runs the kernels"""
    def run():
        topo._components.clear(); topo._loops = None; topo._orientation = None
        return fn()
    return run


def measure(name, v, f, reps):
    f, _, turned = MT.turned_and_shuffled(f, 0.4, seed=1)
    vd, fd = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    topo = MeshTopology(fd, len(v))
    row = {"mesh": name, "faces": len(f), "vertices": len(v), "edges": topo.num_edges, "turned_faces": int(turned.sum()),
           "build_ms": timed(lambda: MeshTopology(fd, len(v)), reps)}
    topo.valence                                                           # the arrays are read once, outside the timed calls
    for c in ("vertex", "edge", "manifold"):
        row[f"components_{c}_ms"] = timed(fresh(topo, lambda c=c: topo.components(c)), reps)
    topo.components("manifold")
    row["orientation_ms"] = timed(lambda: topo._orient(None), reps)       # with the patches' labels kept: the double cover alone
    row["orientation_outward_ms"] = timed(lambda: topo._orient(vd), reps)
    row["border_loops_ms"] = timed(fresh(topo, topo.border_loops), reps)
    flip = topo.orientation()[0]
    row["flipped_faces"], row["border_loops"] = int(flip.sum()), len(topo.border_loops()[1])
    row["components"] = len(topo.components("vertex")[1])
    assert MT.same_direction_manifold_edges(topo.oriented_triangles().cpu().numpy()) == 0
    ev, ef = MT.exploded(v, f)
    evd, efd = torch.from_numpy(ev).cuda(), torch.from_numpy(ef).cuda()
    row["weld_soup_ms"] = timed(lambda: weld_vertices(evd, efd), reps)
    assert weld_vertices(evd, efd)[0].shape[0] == len(v)
    row["host_face_components_ms"] = host_timed(lambda: meshproc.face_components(f, len(v)))
    row["host_border_edge_rows_ms"] = host_timed(lambda: meshproc.border_edge_rows(f))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "meshtopo_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--levels", type=int, nargs="+", default=[5, 6, 7, 8])
    ap.add_argument("--strip", type=int, default=100_000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshtopo_time.py measures on the GPU"
    rows = []
    for level in a.levels:
        rows.append(measure(f"icosphere({level})", *icosphere(level), a.reps))
        print(json.dumps(rows[-1]), flush=True)
    rows.append(measure(f"strip({a.strip})", *MT.strip(a.strip), a.reps))
    print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "what": "medians of repeated calls after warm-up; device rows by events on the stream, host rows by wall clock",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
