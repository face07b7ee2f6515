"""Interleaved wall times of acmmp_main binaries on the synthetic cfg4 folder
(tools/pipeline_times.write_cfg4_dense): each round runs every binary once,
in order, into its own output folder; the last round's output trees are then
compared byte for byte against the first side's.

usage: python tools/cli_ab.py <rounds> <side> [<side> ...] [-- <argument> ...] > cli_ab.jsonl
  side: <binary> or VAR=value@<binary> (one environment variable for that side)
  arguments after --: passed to every side (e.g. --view_parallel)
"""
import filecmp
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def same_tree(a, b):
    """(files compared, relative paths that differ or exist on one side only)."""
    names = sorted({os.path.relpath(os.path.join(d, f), top) for top in (a, b) for d, _, fs in os.walk(top) for f in fs})
    bad = [n for n in names if not (os.path.isfile(os.path.join(a, n)) and os.path.isfile(os.path.join(b, n))
                                    and filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False))]
    return len(names), bad


def main():
    from pipeline_times import write_cfg4_dense
    argv = sys.argv[1:]
    extra = argv[argv.index("--") + 1:] if "--" in argv else []
    argv = argv[:argv.index("--")] if "--" in argv else argv
    rounds, bins = int(argv[0]), argv[1:]
    tmp, dense = write_cfg4_dense(49, 1600, 1200, 20)
    for r in range(rounds):
        for k, side in enumerate(bins):
            env = dict(os.environ)
            b = side
            if "@" in side:
                var, b = side.split("@", 1)
                env[var.split("=", 1)[0]] = var.split("=", 1)[1]
            out = "/ACMMP_ab%d" % k
            shutil.rmtree(dense + out, ignore_errors=True)
            t0 = time.perf_counter()
            subprocess.run([b, dense, "--output_dir", out, "--no_fusion", "--quiet"] + extra, check=True, env=env)
            print(json.dumps({"round": r, "side": side, "s": round(time.perf_counter() - t0, 2)}), flush=True)
    for k in range(1, len(bins)):
        n, bad = same_tree(dense + "/ACMMP_ab0", dense + "/ACMMP_ab%d" % k)
        print(json.dumps({"compared": [bins[0], bins[k]], "files": n, "differ": bad}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
