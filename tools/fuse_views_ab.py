"""In-memory fusion against the folder call on cfg4-shaped maps: the synthetic
cfg4 folder (pipeline_times.write_cfg4_dense), then interleaved rounds, each
run a fresh process with the device already started:

  fuse    ViewParallelPipeline.run(), then the in-process time of
          .fuse(ply=True) alone, split into its phases (image decode, upload
          of the colours, enqueue + the one wait, download, PLY write)
  folder  acmmp_run_fusion_jacobi over the folder that run wrote (with
          ACMMP_LIB=<a parent build> in `folder_env`: the parent's library)

usage: python tools/fuse_views_ab.py [rounds] [folder_env json] [views] [width] [height] [nsrc]
Prints one JSON line per run (points, seconds, phases, a 64-bit hash of the
cloud: of the returned tensors laid out as PLY records for `fuse`, of the PLY's
payload for `folder`) and a last line with the medians and whether the counts
and hashes agree.

  python tools/fuse_views_ab.py --trace <dense> <output_dir>
is the child for a kernel-trace run: the folder's maps loaded into tensors and
one fusion.fuse_views call, nothing else on the device meanwhile.
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def digest(data) -> str:
    return hashlib.blake2b(data, digest_size=8).hexdigest()


def child_fuse(dense, out_dir):
    import numpy as np
    import torch
    from acmmp_amd.distributed import ViewParallelPipeline
    pipe = ViewParallelPipeline(dense, out_dir, device=0)
    pipe.run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz, normal, rgb = pipe.fuse()
    s = time.perf_counter() - t0
    rec = np.empty((len(xyz), 27), np.uint8)
    rec[:, :12] = xyz.cpu().numpy().view(np.uint8).reshape(-1, 12)
    rec[:, 12:24] = normal.cpu().numpy().view(np.uint8).reshape(-1, 12)
    rec[:, 24:] = rgb.cpu().numpy()
    finite = bool(torch.isfinite(xyz).all())  # (the PLY zeroes a point that is not)
    print(json.dumps({"points": len(xyz), "s": round(s, 4), "hash": digest(rec.tobytes()), "finite": finite,
                      "phases": {k[5:]: round(v, 4) for k, v in pipe.phase_s.items() if k.startswith("fuse_")}}))


def child_folder(dense, out_dir):
    import torch
    from acmmp_amd import _abi, pipeline
    _abi.load_library()
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipeline.run_fusion(dense, dense + out_dir, order="jacobi")
    s = time.perf_counter() - t0
    data = open(os.path.join(dense + out_dir, "ACMMP_model.ply"), "rb").read()
    print(json.dumps({"points": n, "s": round(s, 4), "hash": digest(data[data.index(b"end_header\n") + 11:])}))


def child_trace(dense, out_dir):
    import numpy as np
    import torch
    from acmmp_amd import fusion, io as aio, pipeline
    dev = torch.device("cuda", 0)
    problems = pipeline.generate_sample_list(dense)
    index = {p.ref_image_id: i for i, p in enumerate(problems)}
    views = []
    for p in problems:
        rf = aio.result_folder(dense + out_dir, p.ref_image_id)
        depth, normal = aio.read_dmb(os.path.join(rf, "depths_geom.dmb")), aio.read_dmb(os.path.join(rf, "normals.dmb"))
        cam = aio.read_camera(os.path.join(dense, "cams", "%08d_cam.txt" % p.ref_image_id))
        bgr = aio.read_image_bgr(os.path.join(dense, "images", "%08d.jpg" % p.ref_image_id))
        assert bgr.shape[:2] == depth.shape
        planes = torch.from_numpy(np.concatenate([normal, depth[..., None]], -1).astype(np.float32)).to(dev)
        views.append(fusion.FusionView.from_planes(planes, cam, [index[s] for s in p.sources],
                                                   bgr=torch.from_numpy(bgr).to(dev)))
    torch.cuda.synchronize()
    xyz, _, _ = fusion.fuse_views(views)
    print(json.dumps({"points": len(xyz), "views": len(views)}))


def main():
    a = sys.argv
    if len(a) > 1 and a[1] in ("--fuse", "--folder", "--trace"):
        return {"--fuse": child_fuse, "--folder": child_folder, "--trace": child_trace}[a[1]](a[2], a[3])
    from pipeline_times import write_cfg4_dense
    rounds = int(a[1]) if len(a) > 1 else 5
    folder_env = json.loads(a[2]) if len(a) > 2 else {}
    V, W, H, NSRC = (int(a[k]) if len(a) > k else d for k, d in zip(range(3, 7), (49, 1600, 1200, 20)))
    tmp, dense = write_cfg4_dense(V, W, H, NSRC)
    keep = os.environ.get("FUSE_VIEWS_AB_KEEP")  # a file to leave the folder's path in (for a trace run after this)
    runs = {"fuse": [], "folder": []}
    for r in range(rounds):
        for mode in ("fuse", "folder"):  # (fuse first: its run writes the folder the folder call reads)
            env = dict(os.environ, **(folder_env if mode == "folder" else {}))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--" + mode, dense, "/ACMMP_fv"],
                               capture_output=True, text=True, env=env)
            if p.returncode:
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit(p.returncode)
            res = json.loads(p.stdout.strip().splitlines()[-1])
            runs[mode].append(res)
            print(json.dumps({"round": r, "mode": mode, "env": folder_env if mode == "folder" else {}, **res}),
                  flush=True)

    def stats(v):
        v = sorted(v)
        return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}

    phases = {k: stats([x["phases"][k] for x in runs["fuse"]]) for k in runs["fuse"][0]["phases"]}
    every = runs["fuse"] + runs["folder"]
    print(json.dumps({"views": V, "width": W, "height": H, "nsrc": NSRC, "rounds": rounds,
                      "fuse_s": stats([x["s"] for x in runs["fuse"]]), "fuse_phases_s": phases,
                      "folder_s": stats([x["s"] for x in runs["folder"]]),
                      "points": every[0]["points"],
                      "points_agree": len({x["points"] for x in every}) == 1,
                      "hashes_agree": len({x["hash"] for x in every}) == 1}), flush=True)
    if keep:
        open(keep, "w").write(dense)
    else:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
