"""Measurements of profiles/render_mesh/README.md, one process:  python profiles/render_mesh/measure.py [out.json]

  * frame time of phc_render on the H1 capsule scene against phc_render_mesh on H1 carrying 20 subdivision-5 ellipsoids (409 600 triangles),
    for the builder's leaf sizes 2 / 4 / 8: one 640 x 480 view, HIP events, 50 alternated repeats after a warm-up;
  * the viewer's end-to-end throughput (lookup, render, read-back, PNG writing) for 4 tiles of 640 x 480.
The scenes come from the test helpers (tests/render_oracle.py, tests/render_mesh_oracle.py): seeded poses, generated meshes."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

W, H, REPEATS, WARMUP = 640, 480, 50, 5


def main():
    import render_mesh_oracle as rmo
    import render_oracle as ro
    from phc_amd import _lib as L
    from phc_amd import render as R
    from phc_amd import render_mesh as RM
    from phc_amd import view_motion as vm
    lib = L.load()
    sc = ro.make_scene("h1", W=W, H=H)
    caps = torch.from_numpy(np.ascontiguousarray(np.concatenate([sc["capsules"], sc["owner"][..., None].astype(np.float32)], -1).reshape(1, -1), np.float32)).cuda()
    bs = torch.from_numpy(sc["body_state"]).cuda()
    scene = R.scene_struct(caps, bs.shape[0], bs.shape[1], bs)
    env, (eye, tgt, up, fov) = sc["cameras"][0]
    cam = R.Camera(eye, tgt, up, np.degrees(fov))
    meshes, instances = rmo._body_ellipsoids(sc, 5, rng=np.random.default_rng(0))
    sets = {}
    for leaf in (2, 4, 8):
        t0 = time.perf_counter()
        ms = RM.MeshSet(leaf_size=leaf)
        for v, f in meshes:
            ms.add_mesh(v, f)
        for i in instances:
            ms.add_instance(i["mesh"], i["owner"], i["pos"], i["quat"], i["rgb"])
        sets[leaf] = ms.upload("cuda")
        print(f"leaf {leaf}: {ms.struct.num_triangles} triangles, {ms.struct.num_nodes} nodes, {len(instances)} instances, built in {time.perf_counter() - t0:.1f} s", flush=True)
    variants = {"phc_render (capsules)": lambda: R.render(scene, [cam], [env], W, H, lib=lib)}
    for leaf, ms in sets.items():
        variants[f"phc_render_mesh leaf {leaf}"] = (lambda ms=ms: RM.render(scene, ms, [cam], [env], W, H, lib=lib))
    times = {k: [] for k in variants}
    for r in range(WARMUP + REPEATS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARMUP:
                times[name].append(a.elapsed_time(b) * 1e3)
    out = {"frame_us": {k: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for k, v in times.items()}}
    mesh_px = int((RM.render(scene, sets[4], [cam], [env], W, H, hit_id=True, lib=lib)[1] >= L.RENDER_MESH_ID).sum())
    out["mesh_hit_pixels"] = mesh_px
    # viewer throughput, 4 tiles
    with tempfile.TemporaryDirectory() as d:
        argv = ["env.motion_file=synthetic:4:0", "+render.video=" + d, f"+render.width={W}", f"+render.height={H}", "+replay.clips=4", "+replay.frames=120"]
        task = vm.make_task(argv)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = vm.main(argv, task=task)
        dt = time.perf_counter() - t0
        out["viewer"] = {"tiles": 4, "frames": res["frames"], "seconds": dt, "frames_per_second": res["frames"] / dt}
    print(json.dumps(out), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
