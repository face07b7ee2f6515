"""CPU tier of the patch-geometry feature (patch_size / radius_increment other
than 11 / 2): the boundary structs, the envelope rule and the command line
without a device, and resource guards for the general-patch sweep kernel
(hipcc cross-compiles the general u8 unit to a gfx950 listing, as
`make resource-general` does)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from acmmp_amd import _abi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "acmmp_amd", "csrc")
EXE = os.path.join(ROOT, "acmmp_amd", "lib", "acmmp_main")
HIPCC = "/opt/rocm/bin/hipcc"


# ---------------------------------------------------------------------- ABI
def test_pass_options_layout():
    """The two fields came out of reserved[]: same size, same offsets before."""
    assert C.sizeof(_abi.PassOptions) == 16 * 4
    assert _abi.PassOptions.verbose.offset == 10 * 4
    assert _abi.PassOptions.patch_size.offset == 11 * 4
    assert _abi.PassOptions.radius_increment.offset == 12 * 4
    assert _abi.PassOptions.reserved.offset == 13 * 4 and _abi.PassOptions.reserved.size == 3 * 4
    header = open(os.path.join(ROOT, "include", "acmmp.h")).read()
    body = header[header.index("typedef struct acmmp_pass_options"):header.index("} acmmp_pass_options;")]
    fields = re.findall(r"^\s*u?int32_t\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [(n, int(k or 1)) for n, k in fields] == [(n, getattr(t, "_length_", 1)) for n, t in
                                                     _abi.PassOptions._fields_]


def test_pass_options_defaults():
    o = pipeline.pass_options()
    assert (o.patch_size, o.radius_increment) == (0, 0)  # 0: the defaults 11 / 2
    o = pipeline.pass_options(patch_size=7, radius_increment=1)
    assert (o.patch_size, o.radius_increment) == (7, 1)


@pytest.mark.parametrize("patch_size,inc,ok", [
    (0, 0, True), (11, 2, True), (0, 3, True), (7, 0, True),      # 0 maps to 11 / 2
    (3, 1, True), (3, 2, True), (3, 3, False),                    # radius 1: increments 1..2
    (2, 1, True), (1, 1, False), (-3, 1, False),                  # radius >= 1
    (21, 1, True), (21, 20, True), (21, 21, False), (22, 1, False), (23, 2, False),  # radius <= 10
    (8, 3, True), (12, 5, True), (7, 7, False), (7, -1, False),
])
def test_envelope_rule(patch_size, inc, ok):
    assert bool(_abi.load_library().acmmp_patch_geometry_supported(patch_size, inc)) == ok


@pytest.mark.parametrize("args", [["--patch_size", "23"], ["--patch_size", "1"], ["--radius_increment", "0"],
                                  ["--patch_size", "7", "--radius_increment", "7"]])
def test_cli_rejects_outside_envelope_before_any_work(tmp_path, args):
    """No file of the (empty) dense folder is read and no device is opened:
    the answer is the usage error, with the envelope in the message."""
    r = subprocess.run([EXE, str(tmp_path)] + args + ["--no_fusion", "--quiet"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "outside the built envelope: 1 <= patch_size / 2 <= 10" in r.stderr
    assert os.listdir(tmp_path) == []


def test_cli_help_lists_the_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--patch_size N" in r.stdout and "--radius_increment N" in r.stdout


# --------------------------------------------------------------- ISA guards
# scratch per lane of each bucket of k_sweep_g<NS, u8> as first built (cost_array[8][NS]
# dominates, as in k_sweep_f): a regression ceiling, not a target
SCRATCH_MAX = {9: 384, 16: 624, 20: 768, 32: 1200}
LDS_MAX = 160 * 1024 // 2  # two 256-thread blocks per CU (2 waves/SIMD), tests/test_isa_guards.py's bound


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa_g") / "dev_kernels_g.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fno-slp-vectorize", "-I../../include", "-DACMMP_TX_UNIT=2", "-DACMMP_GENERAL_UNIT",
           "--cuda-device-only", "-S", "acmmp_kernels_tx.hip", "-o", str(out),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = out.read_text().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN5acmmp9k_sweep_gILi9ELi2EE\S*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    return lines[start:end + 1], r.stderr


def test_no_flat_loads_in_general_sweep(listing):
    body, _ = listing
    flat = [l.strip() for l in body if re.match(r"\s+flat_load", l)]
    assert not flat, flat[:5]


@pytest.mark.parametrize("ns", sorted(SCRATCH_MAX))
def test_general_sweep_resources(listing, ns):
    _, remarks = listing
    tag = f"Function Name: _ZN5acmmp9k_sweep_gILi{ns}ELi2EE"
    assert tag in remarks, f"k_sweep_g<{ns}, u8> not instantiated"
    sweep = remarks[remarks.index(tag):]
    sweep = sweep[:sweep.index("Function Name:", len(tag))] if "Function Name:" in sweep[len(tag):] else sweep
    occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", sweep).group(1))
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", sweep).group(1))
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", sweep).group(1))
    assert occ == 2 and scratch <= SCRATCH_MAX[ns] and lds <= LDS_MAX, (ns, occ, scratch, lds)
