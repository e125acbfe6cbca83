#!/usr/bin/env python
"""Timing of the mesh cleaning (mm3dgs_mesh_components, mm3dgs_mesh_clean_plan + mm3dgs_mesh_clean_emit; csrc/meshclean.hip) against the
host route through scipy, and the A/B that decides whether find() halves paths.  Needs the GPU; there is no fall-back.

    python tools/mesh_clean_ab.py [--calls 200] [--untimed 20] [--host-calls 5] [--frames 30] [--repeats 3] [--variant LIB] [--out profiles/r18_mesh_clean.jsonl]

Sets: the sensor-view meshes of tools/mesh_ab.py (every frame's colour and sensor depth fused into a 256^3 volume, at 640x480 and 1200x680);
a ribbon -- one strip, one component -- over 2^20 vertices with the vertex indices ascending, descending and shuffled; 10^6 triangles that
are each their own component.

(a) mm3dgs_mesh_components alone, and mm3dgs_mesh_clean_plan + _emit (mode small, 100 triangles, caps from the plan's totals), each between
device events: the median, p10 and p90 of `--calls` calls after `--untimed` (a set on which one call takes more than 20 ms gets fewer calls,
at least 5: the line says how many).  With `--variant LIB` (tools/build_variant.sh nohalving -DMC_PATH_HALVING=0 builds the library
without path halving in find()) the components call of that library is timed on the same buffers in the same process, and its labels are compared.
(b) The host route with its transfers, `--host-calls` times on the host clock: triangles and rows to the host, scipy's connected_components
over the triangle sides, a count per component, boolean masks, the re-index, rows and triangles back to the device.
(c) A whole SLAM.export_mesh over `--frames` sensor views with `mesh.clean` none and small, `--repeats` times after one untimed pass; host
clock, device synchronised at both ends."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
NAMES = ("mm3dgs_mesh_clean_work_bytes", "mm3dgs_mesh_components", "mm3dgs_mesh_clean_plan", "mm3dgs_mesh_clean_emit")


def load_variant(path):
    from mm3dgs_slam_amd import _lib
    lib = C.CDLL(path)
    for name in NAMES + ("mm3dgs_last_error",):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGS[name]
    return lib


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stat(v):
    return dict(median=round(statistics.median(v), 2), p10=round(pct(v, 0.1), 2), p90=round(pct(v, 0.9), 2), calls=len(v))


def timed(fn, calls, untimed):
    """us per call between device events; a call above 20 ms shortens the series"""
    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    first = once()
    if first > 20e3:
        calls, untimed = max(5, min(calls, int(2e6 / first))), 1
    for _ in range(untimed):
        once()
    return stat([once() for _ in range(calls)])


def ribbon(order, n=1 << 20):
    name = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.RandomState(7).permutation(n)}[order]
    i = np.arange(n - 2)
    return n, name[np.stack([i, i + 1, i + 2], 1)].astype(np.int32)


def islands(n=1000000):
    t = np.arange(n)
    return 3 * n, np.stack([t, t + n, t + 2 * n], 1).astype(np.int32)


def sensor_mesh(args, H, W, tmp):
    """(slam, voxel, box, rows, triangles) of tools/mesh_ab.py's sensor-view volume"""
    import mesh_ab
    from mm3dgs_slam_amd import export, mesh as ms
    slam, _ = mesh_ab.start(args, H, W, tmp)
    origin, voxel, trunc, box = mesh_ab.lattice(slam, 1, "sensor")
    vol = ms.TsdfVolume((mesh_ab.SIDE,) * 3, origin, voxel, trunc, H, W, slam.cfg["cam"], sil_min=0.99, device=DEV)
    with torch.no_grad():
        for view in export.views(slam, 1, "sensor", "mesh"):
            vol.add(*view)
    rows, tris, _ = vol.extract()
    return slam, voxel, box, rows, tris


def host_route(rows, tris):
    """the cleaned mesh through scipy on the host, transfers included; returns the two device tensors"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    r, t = rows.cpu().numpy(), tris.cpu().numpy().astype(np.int64)
    V = len(r)
    ok = ((t >= 0) & (t < V)).all(1)
    g = t[ok]
    a, b = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    n, comp = connected_components(coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(V, V)), directed=False)
    count = np.bincount(comp[g[:, 0]], minlength=n)
    vmask = (count >= 100)[comp]
    tmask = ok.copy()
    tmask[ok] = vmask[g[:, 0]]
    new = np.cumsum(vmask) - 1
    return torch.from_numpy(r[vmask]).to(DEV), torch.from_numpy(new[t[tmask]].astype(np.int32)).to(DEV)


def measure_set(args, emit, name, rows, tris, libs):
    from mm3dgs_slam_amd import _lib
    from mm3dgs_slam_amd.rasterizer import _stream
    P = _lib.ptr
    V, T = int(rows.shape[0]), int(tris.shape[0])
    label = {k: torch.empty(max(V, 1), dtype=torch.int32, device=DEV) for k in libs}
    tri_count = torch.empty(max(V, 1), dtype=torch.int32, device=DEV)
    counters = torch.empty(8, dtype=torch.int64, device=DEV)
    line = dict(part="a", set=name, vertices=V, triangles=T)
    for k, lib in libs.items():
        def components(lib=lib, k=k):
            assert lib.mm3dgs_mesh_components(V, T, P(tris), P(label[k]), P(tri_count), P(counters), _stream()) == 0, lib.mm3dgs_last_error()
        line[f"components_us_{k}"] = s = timed(components, args.calls, args.untimed)
        line[f"components_ns_per_triangle_{k}"] = round(s["median"] * 1e3 / max(T, 1), 3)
    if len(libs) > 1:
        line["variant_labels_equal"] = bool(torch.equal(label["product"], label["variant"]))
        line["variant_over_product_median"] = round(line["components_us_variant"]["median"] / line["components_us_product"]["median"], 3)
    lib = libs["product"]
    assert lib.mm3dgs_mesh_components(V, T, P(tris), P(label["product"]), P(tri_count), P(counters), _stream()) == 0
    work = torch.empty(int(lib.mm3dgs_mesh_clean_work_bytes(V, T)) // 8, dtype=torch.int64, device=DEV)
    assert lib.mm3dgs_mesh_clean_plan(V, T, P(tris), P(label["product"]), P(tri_count), 1, 100, P(work), P(counters), _stream()) == 0
    c = counters.cpu().tolist()
    nv, nt = c[5], c[6]
    out_rows, out_tris = torch.empty(max(nv, 1), 4, dtype=torch.int32, device=DEV), torch.empty(max(nt, 1), 3, dtype=torch.int32, device=DEV)
    index = torch.empty(max(nv, 1), dtype=torch.int32, device=DEV)

    def plan_emit():
        assert lib.mm3dgs_mesh_clean_plan(V, T, P(tris), P(label["product"]), P(tri_count), 1, 100, P(work), P(counters), _stream()) == 0
        assert lib.mm3dgs_mesh_clean_emit(V, T, P(rows), P(tris), P(work), P(out_rows), nv, P(out_tris), nt, P(index), P(counters), _stream()) == 0
    line["plan_emit_us"] = timed(plan_emit, args.calls, args.untimed)
    line.update(components=c[0], largest_triangles=c[1] >> 32, kept_vertices=nv, kept_triangles=nt)
    emit(line)
    ms_ = []
    for k in range(args.host_calls + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hr, ht = host_route(rows, tris)
        torch.cuda.synchronize()
        if k:
            ms_.append((time.perf_counter() - t0) * 1e3)
    same = bool(hr.shape[0] == nv and ht.shape[0] == nt and torch.equal(hr, out_rows[:nv]) and torch.equal(ht, out_tris[:nt]))
    emit(dict(part="b", set=name, vertices=V, triangles=T, host_ms=dict(median=round(statistics.median(ms_), 3), min=round(min(ms_), 3), max=round(max(ms_), 3), calls=len(ms_)),
              host_result_equals_device=same))


def export_times(slam, args, emit, shape, voxel, box):
    pad = 5.0 * voxel
    base = dict(slam.cfg.get("mesh") or {}, bounds=[float(v) for v in np.concatenate([box[:3] - pad, box[3:] + pad])], voxel=voxel, every=1, source="sensor")
    line = dict(part="c", shape=shape, frames=args.frames, repeats=args.repeats)
    for clean in ("none", "small"):
        slam.cfg["mesh"] = dict(base, clean=clean, clean_min_triangles=100)
        ms_ = []
        for k in range(args.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = slam.export_mesh()
            torch.cuda.synchronize()
            if k:
                ms_.append((time.perf_counter() - t0) * 1e3)
        line[f"ms_export_clean_{clean}"] = dict(median=round(statistics.median(ms_), 3), min=round(min(ms_), 3), max=round(max(ms_), 3))
        line[f"counters_{clean}"] = out["counters"]
    emit(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--untimed", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=150000, help="size of the synthetic ground-truth scene (bench.py's default)")
    ap.add_argument("--variant", default="", help="a library built with -DMC_PATH_HALVING=0 (tools/build_variant.sh): its components call is timed beside the product's")
    ap.add_argument("--skip-sensor", action="store_true", help="leave the sensor-view meshes and the exports out")
    ap.add_argument("--out", default="", help="append the lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from mm3dgs_slam_amd import _lib
    libs = {"product": _lib.load()}
    if args.variant:
        libs["variant"] = load_variant(args.variant)

    def emit(d):
        d = dict(d, device=torch.cuda.get_device_name(0), **({"variant": os.path.basename(args.variant)} if args.variant and d.get("part") == "a" else {}))
        print(json.dumps(d), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(d) + "\n")

    for order in ("ascending", "descending", "shuffled"):
        V, tris = ribbon(order)
        measure_set(args, emit, f"ribbon 2^20 {order}", torch.zeros(V, 4, dtype=torch.int32, device=DEV), torch.from_numpy(tris).to(DEV), libs)
    V, tris = islands()
    measure_set(args, emit, "10^6 one-triangle components", torch.zeros(V, 4, dtype=torch.int32, device=DEV), torch.from_numpy(tris).to(DEV), libs)
    if args.skip_sensor:
        return
    import mesh_ab
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in mesh_ab.SHAPES:
            slam, voxel, box, rows, tris = sensor_mesh(args, H, W, tmp)
            measure_set(args, emit, f"sensor mesh {W}x{H}", rows, tris, libs)
            export_times(slam, args, emit, f"{W}x{H}", voxel, box)
            del slam, rows, tris
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
