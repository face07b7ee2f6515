"""RunFusion A/B on cfg4-shaped maps: the synthetic cfg4 folder
(pipeline_times.write_cfg4_dense) through the distributed driver once, then
RunFusion in a subprocess per configuration, configurations interleaved
`repeat` times (the host is shared: interleaving spreads its noise).

usage: python tools/fusion_ab.py '<json list of env dicts>' [repeat] [views] [width] [height] [nsrc]
  e.g. '[{}, {"ACMMP_HOST_THREADS": "8"}]'
A configuration's "order" key is not an environment variable: "literal"
(default) or "jacobi" (the device fusion, acmmp_run_fusion_jacobi), e.g.
  '[{"ACMMP_LIB": "<a parent build>"}, {"order": "jacobi"}]'
A configuration's "fusion" key, not an environment variable either, picks the
call: "run" (default, RunFusion) or "prior" (RunPriorAwareFusion, in either
order). With a "prior" configuration the driver runs a second time with another
seed into a second output folder: that reconstruction is the call's output
folder (its maps are the priors), the first one its fusion folder.
Prints one JSON line per run with the fusion's own phase timing line, the
in-process seconds of the call alone (`s`; library load and device start-up
are outside it) and a digest of the PLY's point set; at the end one line with
each configuration's median and the sizes of the one-sided differences between
the first two configurations' point sets.
"""
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def point_records(path):
    """The PLY's 27-byte records, sorted (a point set, order-free)."""
    import numpy as np
    data = open(path, "rb").read()
    body = data[data.index(b"end_header\n") + 11:]
    rec = np.frombuffer(body, np.uint8).reshape(-1, 27)
    return np.unique(np.ascontiguousarray(rec).view([("r", "V27")]).ravel())


def setdiff(a, b):
    import numpy as np
    return np.setdiff1d(a, b)


def main():
    import torch
    from acmmp_amd.distributed import ViewParallelPipeline
    from pipeline_times import write_cfg4_dense
    a = sys.argv
    configs = json.loads(a[1]) if len(a) > 1 else [{}]
    repeat = int(a[2]) if len(a) > 2 else 3
    V, W, H, NSRC = (int(a[k]) if len(a) > k else d for k, d in zip(range(3, 7), (49, 1600, 1200, 20)))
    tmp, dense = write_cfg4_dense(V, W, H, NSRC)
    ViewParallelPipeline(dense, "/ACMMP_fab", device=0).run()
    if any(cfg.get("fusion") == "prior" for cfg in configs):
        ViewParallelPipeline(dense, "/ACMMP_fab2", device=0, seed=4321).run()
    torch.cuda.synchronize()
    # (the jacobi call is preceded by a device start-up outside the timed call: torch, already
    # imported by the package loader, creates the context)
    code = ("import sys, time, json; sys.path.insert(0, %r); from acmmp_amd import pipeline, _abi; "
            "_abi.load_library(); import torch; torch.zeros(1, device='cuda'); torch.cuda.synchronize(); "
            "kw = {'order': 'jacobi'} if sys.argv[1] == 'jacobi' else {}; d, out, out2 = %r, %r, %r; "
            "t0 = time.perf_counter(); "
            "n = pipeline.run_prior_aware_fusion(d, out2, out, **kw) if sys.argv[2] == 'prior' else "
            "pipeline.run_fusion(d, out, **kw); "
            "print(json.dumps({'points': n, 's': round(time.perf_counter() - t0, 3)}))"
            % (ROOT, dense, dense + "/ACMMP_fab", dense + "/ACMMP_fab2"))
    plys = {"run": os.path.join(dense + "/ACMMP_fab", "ACMMP_model.ply"),
            "prior": os.path.join(dense + "/ACMMP_fab2", "ACMMP_prior_model.ply")}
    times, sets = {}, {}
    for r in range(repeat):
        for k, cfg in enumerate(configs):
            cfg = dict(cfg)
            order, fusion = cfg.pop("order", "literal"), cfg.pop("fusion", "run")
            env = dict(os.environ, ACMMP_HOST_TIMING="1", **cfg)
            p = subprocess.run([sys.executable, "-c", code, order, fusion], capture_output=True, text=True, env=env)
            if p.returncode:
                print(p.stderr[-2000:], file=sys.stderr)
                raise SystemExit(p.returncode)
            res = json.loads(p.stdout.strip().splitlines()[-1])
            timing = [l for l in p.stderr.splitlines() if l.startswith(("[RunFusion", "[RunPriorAwareFusion"))]
            times.setdefault(k, []).append(res["s"])
            if k not in sets:
                sets[k] = point_records(plys[fusion])
            print(json.dumps({"round": r, "config": k, "fusion": fusion, "order": order, "env": cfg, **res,
                              "timing": timing[-1] if timing else None}), flush=True)
    summary = {"median_s": {k: sorted(v)[len(v) // 2] for k, v in times.items()},
               "points": {k: len(v) for k, v in sets.items()}}
    if len(sets) > 1:
        summary["only_in_config_0"] = len(setdiff(sets[0], sets[1]))
        summary["only_in_config_1"] = len(setdiff(sets[1], sets[0]))
    print(json.dumps(summary), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
